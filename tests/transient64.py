"""Float64 references for DECOMPOSED films -- transient, bounce, modulated -- of the scenes only the EXTRA / AREA kernels render: spot, area
(rectangle, disk, sphere), environment-map and lens scenes.  Plain numpy; the domain is that of tests/volpath64_all.py and
tests/volpath64_shapes.py: index 1, a homogeneous grey medium with a Henyey-Greenstein phase function in the index-matched cube [-1, 1]^3,
straight rays, a box filter of half a pixel, no Russian roulette.

THE PATH-LENGTH RULE, and where it comes from.  Not from the kernels: from include/mer.h (mer_scene_desc.decomposition: "every radiance
contribution is binned by its optical path length ... calibrated_transient != 0 leaves the camera edge out of the path length ... Bounce:
the same film, binned by the number of path edges instead -- every edge counts 1.0 where transient adds its optical length"; .sensor: the
primary ray starts at the ray origin of the sensor, on the aperture for the lens kinds; n_emitters: "the nearest one ends a ... look-up"),
DESIGN.md section 1 "Transient film (N1)" (camera edge + sum of the free-flight segments + the connecting segment: the NEE / look-up walk to
the boundary, or the connection's distance; bin floor((l - minBound) / binWidth), dropped outside [0, frames); calibratedTransient drops
the camera edge from a TRANSIENT film only) and the reference's bdpt_proc.cpp:151-187 (sensorPathlength[i] = sensorPathlength[i - 1] +
edge(i - 1).length x refIndex from startIndex 2, or 3 when calibrated; the bounce loop adds 1.0 per edge from i = 2 whatever the flag).
Restated for the volpath estimator:
  - the camera edge runs from the ray origin tests/sensors64.sensor_rays returns to the first point on the cube, or to a directly seen
    emitter shape; a ray that sees the environment directly has none.  `calibrated` drops it from a transient film, never from a bounce film;
  - every segment between vertices counts in full (the chord of an unscattered path included; what such a path then meets outside -- a
    shape -- prolongs that last edge by the free-space leg: length in a transient film, no further edge in a bounce film, because the
    index-matched boundary is no vertex);
  - the connecting edge to a point, spot, rectangle, disk or sphere sample is the full vertex-to-emitter distance;
  - a look-up that ends on a shape counts vertex to shape;
  - a look-up or luminaire sample that ends in the environment (a constant or a map) counts vertex to the cube's exit;
  - a bounce film counts 1 per edge wherever the transient film adds a length: a path of k scatterings lands in frame k + 2 of a film
    over [0, F) with unit bins (camera edge, k segments, one connection or look-up), an unscattered path through the cube in frame 2, a
    directly seen shape in frame 1, the directly seen environment in frame 0;
  - a modulated film has one frame and weights every contribution by correlation(length), with no bounds.
max_depth is volpath's (mer.h: "the null boundary costs one depth"; "the null crossing of a connection counts against max_depth with
straight rays"): vertex k may scatter and connect inside the cube when k + 2 <= max_depth, and connect or look up ACROSS the boundary when
k + 3 <= max_depth; the unscattered path through the cube needs 3.  Exactly one scattering vertex is max_depth = 3 for an emitter inside the
cube and 4 for one outside it.

`render` is the estimator of tests/volpath64_all.py -- every point, spot and shape sampled at every vertex, the environment's luminaire
sample, the phase sample and its look-up, power heuristic -- over the emitter shapes of tests/volpath64_shapes.py (Planar, Sphere;
volpath64_multi.Rect is converted), with the length of every contribution carried along.  One walk can be binned into several films at once
(`films`): the walk does not depend on the bookkeeping.  `wrong` builds the films the discrimination tests must tell apart:
  "edge_from_exit"      every connecting edge to a point, spot or shape (sample or look-up) is measured from where it leaves the cube;
  "calibrated_ignored"  the camera edge always counts;
  "bounce_counts_exit"  a connection or look-up that crosses the null boundary counts 2.

The single-scatter quadratures (spot_profile, shape_profile, map_profile) integrate along the central ray of the pencil camera of
tests/closed_form.single_scatter_scene: the two MIS strategies of a renderer sum to their integrands, so no weights appear."""
import functools

import numpy as np
from tests import ref64, sensors64 as S, volpath64_multi as vm, volpath64_shapes as vs
from tests.envmap64 import EnvMap64

WRONG = (None, "edge_from_exit", "calibrated_ignored", "bounce_counts_exit")


# ------------------------------------------------------------------------------------------------ films

class Spec:
    """how one film bins the walk: frames = (min_bound, bin_width, F); mode "transient" | "bounce"; weight(length) collapses it to one frame"""

    def __init__(self, frames=(0.0, 1.0, 1), mode="transient", calibrated=False, weight=None, wrong=None, max_depth=-1):
        assert mode in ("transient", "bounce") and wrong in WRONG
        self.lo, self.bw, self.F = float(frames[0]), float(frames[1]), (1 if weight is not None else int(frames[2]))
        self.mode, self.calibrated, self.weight, self.wrong, self.D = mode, bool(calibrated), weight, wrong, int(max_depth)

    def lengths(self, cam, camn, seg, segn, conn, conn_x, connn, cross):
        if self.mode == "bounce":
            return camn + segn + connn * np.where(cross & (self.wrong == "bounce_counts_exit"), 2.0, 1.0)
        drop = self.calibrated and self.wrong != "calibrated_ignored"
        return (0.0 if drop else cam) + seg + (conn_x if self.wrong == "edge_from_exit" else conn)


class Film:
    """what `render` returns per Spec.  A cell is one frame of one block x block pixel block; a cell's value is the SUM of its pixels' means.
    mean [nb, F], cov [nb, F, F] (covariance of those means between the frames of a block: what pooling frames needs), tot [F], tot_cov [F, F]
    (the whole image), pix / pix_var [H, W] (all frames summed: the one frame of a modulated film), steady [H, W] (every contribution, binned
    or not, unweighted), spp"""

    def __init__(self, **kw):
        self.__dict__.update(kw)

    @property
    def var(self):
        return np.einsum("bff->bf", self.cov)

    @property
    def tot_var(self):
        return np.diag(self.tot_cov)

    @property
    def tail(self):
        """the share of the energy that fell outside [min_bound, max_bound)"""
        return 1.0 - self.pix.sum() / self.steady.sum()


class _Acc:
    def __init__(self, spec, width, height, block):
        self.s, self.w, self.h, self.b = spec, width, height, block
        nb, F = (width // block) * (height // block), spec.F
        self.m1 = np.zeros((nb, F)); self.m2 = np.zeros((nb, F, F)); self.t1 = np.zeros(F); self.t2 = np.zeros((F, F))
        self.p1 = np.zeros(width * height); self.p2 = np.zeros(width * height); self.s1 = np.zeros(width * height)

    def begin(self, N):
        self.A = np.zeros((N, self.s.F)); self.L = np.zeros(N)

    def add(self, idx, val, kmin, *edges):
        s = self.s
        v = val if s.D < 0 else np.where(kmin <= s.D, val, 0.0)
        self.L[idx] += v
        ln = np.broadcast_to(s.lengths(*edges), v.shape)
        if s.weight is not None:
            self.A[idx, 0] += v * np.asarray(s.weight(ln), np.float64)
            return
        b = np.floor((ln - s.lo) / s.bw)
        m = (b >= 0) & (b < s.F) & (v != 0)
        self.A[idx[m], b[m].astype(np.int64)] += v[m]

    def end(self, k):
        w, h, b, F = self.w, self.h, self.b, self.s.F
        Y = self.A.reshape(k, h // b, b, w // b, b, F).sum((2, 4)).reshape(k, -1, F)
        self.m1 += Y.sum(0); self.m2 += np.einsum("kbf,kbg->bfg", Y, Y)
        Yt = self.A.reshape(k, -1, F).sum(1)
        self.t1 += Yt.sum(0); self.t2 += Yt.T @ Yt
        P = self.A.sum(1).reshape(k, -1)
        self.p1 += P.sum(0); self.p2 += (P * P).sum(0); self.s1 += self.L.reshape(k, -1).sum(0)

    def film(self, spp):
        m = self.m1 / spp; t = self.t1 / spp; p = self.p1 / spp
        return Film(mean=m, cov=(self.m2 / spp - np.einsum("bf,bg->bfg", m, m)) / spp, tot=t, tot_cov=(self.t2 / spp - np.outer(t, t)) / spp,
                    pix=p.reshape(self.h, self.w), pix_var=((self.p2 / spp - p * p) / spp).reshape(self.h, self.w),
                    steady=(self.s1 / spp).reshape(self.h, self.w), spp=spp, spec=self.s)


def as_shape(s):
    """volpath64_multi.Rect -> volpath64_shapes.Planar (the same rectangle, the same side)"""
    if isinstance(s, vm.Rect):
        return vs.Planar(np.stack([s.u, s.v, s.n, s.o], 1), s.L, False)
    return s


def _outside(shapes, env, o, d, t0, ch):
    """what a ray that has left the cube at o meets: (radiance, the solid-angle pdf -- from the point t0 behind o -- of the strategy that samples
    it, the distance to the shape or inf for the environment)"""
    k, t = vs._nearest(shapes, o, d)
    if isinstance(env, EnvMap64):
        Le, pdf = env.eval(d)
        L = Le[:, ch].copy(); pdf = pdf.copy()
    else:
        L = np.full(len(o), float(env)); pdf = np.full(len(o), vm.INV_FOURPI)
    for j, s in enumerate(shapes):
        m = k == j
        if m.any():
            c = np.sum(d[m] * s.normal(o[m] + d[m] * t[m, None]), 1)
            L[m] = np.where(c < 0, s.L, 0.0)
            pdf[m] = np.where(c < 0, vs._area_pdf(s, t[m] + t0[m], c), 0.0)
    return L, pdf, t


def render(kind, points, spots, shapes, env, sigma_s, sigma_a, g, width, height, fov_x_deg, cam_to_world, aperture_radius=0.0, focus_distance=1.0,
           near=1e-2, far=1e4, spp=2048, seed=0, chunk=128, max_bounces=60, hide_emitters=False, channel=0, block=4,
           frames=(0.0, 1.0, 1), mode="transient", calibrated=False, weight=None, wrong=None, max_depth=-1, films=None):
    """kind: sensors64 kind; points: [(position, intensity)]; spots: [volpath64_spot.Spot]; shapes: [Rect | Planar | Sphere]; env: a float or
    an EnvMap64 (its `channel`).  -> the Film of (frames, mode, calibrated, weight, wrong, max_depth), or one Film per Spec of `films`"""
    specs = [Spec(frames, mode, calibrated, weight, wrong, max_depth)] if films is None else list(films)
    block = min(block, width, height)
    assert width % block == 0 and height % block == 0
    accs = [_Acc(s, width, height, block) for s in specs]
    shapes = [as_shape(s) for s in shapes]
    rng = np.random.default_rng(seed)
    st = sigma_s + sigma_a
    npx = width * height
    is_map = isinstance(env, EnvMap64)
    lights = [(np.asarray(p, np.float64), float(i), None) for p, i in points] + [(s.position, s.I, s) for s in spots]
    deepest = -1 if any(s.D < 0 for s in specs) else max(s.D for s in specs)

    def add(idx, val, kmin, *edges):
        for a in accs:
            a.add(idx, val, kmin, *edges)

    for c0 in range(0, spp, chunk):
        k = min(chunk, spp - c0)
        pix = np.tile(np.arange(npx), k)
        N = len(pix)
        for a in accs:
            a.begin(N)
        pos = np.stack([pix % width, pix // width], 1) + rng.random((N, 2))
        u = rng.random((N, 2)) if kind in (S.THINLENS, S.TELECENTRIC) else None
        o, d, _, _ = S.sensor_rays(kind, cam_to_world, width, height, fov_x_deg, near, far, pos, u, aperture_radius, focus_distance)
        tn, tf = vm._slabs(o, d)
        cube = (tn <= tf) & (tf > 0)
        tcube = np.where(cube, np.maximum(tn, 0.0), np.inf)
        Lo, _, tsh = _outside(shapes, env, o, d, np.zeros(N), channel)
        first = ~cube | (tsh < tcube)                                           # the ray ends on a shape or escapes
        if not hide_emitters:
            i = np.where(first)[0]; on = np.isfinite(tsh[i])
            add(i, Lo[i], 1, np.where(on, tsh[i], 0.0), on.astype(np.float64), 0.0, 0.0, 0.0, 0.0, 0.0, False)
        idx = np.where(~first)[0]
        x = o[idx] + d[idx] * tcube[idx, None]; dirn = d[idx]; T = np.ones(len(idx)); cam = tcube[idx]; seg = np.zeros(len(idx))
        for v in range(1, max_bounces + 2):                                     # v: the number of the vertex this flight may end in
            if len(idx) == 0:
                break
            tex = vm._exit(x, dirn)
            tfl = -np.log1p(-rng.random(len(idx))) / st
            scat = tfl < tex
            if v == 1 and not hide_emitters:                                    # the unscattered path leaves: what it meets outside
                lv = ~scat
                if lv.any():
                    Lo, _, t = _outside(shapes, env, x[lv] + dirn[lv] * tex[lv, None], dirn[lv], np.zeros(lv.sum()), channel)
                    leg = np.where(np.isfinite(t), t, 0.0)
                    add(idx[lv], T[lv] * Lo, 3, cam[lv], 1.0, tex[lv], 1.0, leg, leg, 0.0, False)
            idx, x, dirn, T, cam, seg = idx[scat], x[scat] + dirn[scat] * tfl[scat, None], dirn[scat], T[scat] * (sigma_s / st), cam[scat], seg[scat] + tfl[scat]
            n = len(idx)
            if n == 0 or (deepest >= 0 and v + 2 > deepest):
                break
            inside, across = v + 2, v + 3                                       # the least max_depth that allows a connection of this vertex
            for p, inten, spot in lights:                                       # points and spots: all of them
                dv = p - x; r = np.linalg.norm(dv, axis=1); dv /= r[:, None]
                fall = 1.0 if spot is None else spot.falloff(dv)
                f = ref64.hg_pdf(g, np.sum(dirn * dv, 1))
                te = vm._exit(x, dv); cross = r > te
                add(idx, T * inten * fall / (r * r) * np.exp(-st * np.minimum(r, te)) * f, np.where(cross, across, inside),
                    cam, 1.0, seg, float(v), r, np.where(cross, r - te, r), 1.0, cross)
            if is_map or env != 0:                                              # the environment's luminaire sample, blocked by any shape
                if is_map:
                    _, _, de, vop, epdf = env.sample(rng.random((n, 2)))
                    vop = vop[:, channel]
                else:
                    w = rng.random((n, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(1 - z * z)
                    de = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
                    epdf = np.full(n, vm.INV_FOURPI); vop = np.full(n, float(env) / vm.INV_FOURPI)
                blocked = vs._nearest(shapes, x, de)[0] >= 0
                f = ref64.hg_pdf(g, np.sum(dirn * de, 1))
                te = vm._exit(x, de)
                with np.errstate(divide="ignore", invalid="ignore"):
                    w = np.where((epdf > 0) & ~blocked, vm._mis(epdf, f), 0.0)
                add(idx, T * np.exp(-st * te) * f * w * vop, across, cam, 1.0, seg, float(v), te, te, 1.0, True)
            for j, s in enumerate(shapes):                                      # every shape, each blocked by the others in front of the sampled point
                dv, dist, nq = s.sample(x, rng.random((n, 2)))
                c = np.sum(dv * nq, 1)
                pdf = vs._area_pdf(s, dist, c)
                blocked = np.zeros(n, bool)
                for i, q in enumerate(shapes):
                    if i != j:
                        blocked |= q.intersect(x, dv) < dist
                f = ref64.hg_pdf(g, np.sum(dirn * dv, 1))
                te = vm._exit(x, dv)
                add(idx, np.where(blocked | (c >= 0), 0.0, T * s.L / pdf * np.exp(-st * te) * f * vm._mis(pdf, f)), across,
                    cam, 1.0, seg, float(v), dist, dist - te, 1.0, True)
            wo = vm._hg_sample(g, dirn, rng.random((n, 2)))                     # the phase sample and the look-up along it
            f = ref64.hg_pdf(g, np.sum(dirn * wo, 1))
            te = vm._exit(x, wo)
            Lo, epdf, t = _outside(shapes, env, x + wo * te[:, None], wo, te, channel)
            on = np.isfinite(t)
            add(idx, T * np.exp(-st * te) * vm._mis(f, epdf) * Lo, across, cam, 1.0, seg, float(v), te + np.where(on, t, 0.0), np.where(on, t, te), 1.0, True)
            dirn = wo
        for a in accs:
            a.end(k)
    out = [a.film(spp) for a in accs]
    return out[0] if films is None else out


# ------------------------------------------------------------------------------------------------ the acceptance rule on cells

class Batches:
    """B independent renders of a decomposed film, [B, H, W, F] per-pixel frame values: cells, totals and their variances from the batches"""

    def __init__(self, x, block=4):
        x = np.asarray(x, np.float64)
        B, h, w, F = x.shape
        b = min(block, w, h)
        self.B = B
        self.cells = x.reshape(B, h // b, b, w // b, b, F).sum((2, 4)).reshape(B, -1, F)
        self.totals = x.reshape(B, -1, F).sum(1)
        self.pixels = x.sum(3)

    def group(self, b, f0, f1):
        y = self.cells[:, b, f0:f1].sum(1)
        return y.mean(), y.var(ddof=1) / self.B

    def frame_totals(self):
        return self.totals.mean(0), self.totals.var(0, ddof=1) / self.B

    def per_pixel(self):
        return self.pixels.mean(0), self.pixels.var(0, ddof=1) / self.B


def _group(a, b, f0, f1):
    if isinstance(a, Batches):
        return a.group(b, f0, f1)
    return a.mean[b, f0:f1].sum(), a.cov[b, f0:f1, f0:f1].sum()


def _totals(a):
    return a.frame_totals() if isinstance(a, Batches) else (a.tot, a.tot_var)


def per_pixel(a):
    return a.per_pixel() if isinstance(a, Batches) else (a.pix, a.pix_var)


def _pools(mean, cov):
    pools = []; f0 = 0
    for f in range(len(mean)):
        m = mean[f0:f + 1].sum(); v = cov[f0:f + 1, f0:f + 1].sum()
        if m > 0 and np.sqrt(max(v, 0.0)) < 0.25 * m:
            pools.append((f0, f + 1)); f0 = f + 1
    return pools, mean[f0:].sum()


def tested_cells(ref):
    """the pooling rule, on the reference alone: a cell is tested when the reference's standard error is below 25 % of its mean; one that is
    not is pooled with the next frame of its block until it is.  -> ([(block, first frame, one past the last)], the share of the reference
    film's total that stays untested)"""
    groups = []; left = 0.0
    for b in range(ref.mean.shape[0]):
        pools, rest = _pools(ref.mean[b], ref.cov[b])
        groups += [(b, f0, f1) for f0, f1 in pools]; left += rest
    return groups, left / ref.mean.sum()


def tested_frames(ref):
    """tested_cells for the frame totals of the whole image: ([(first frame, one past the last)], the untested share)"""
    pools, rest = _pools(ref.tot, ref.tot_cov)
    return pools, rest / ref.tot.sum()


def tested(ref):
    """what `compare` tests, formed on the right reference alone: (tested_cells, tested_frames) without their shares"""
    return tested_cells(ref)[0], tested_frames(ref)[0]


def _total(a, f0, f1):
    if isinstance(a, Batches):
        y = a.totals[:, f0:f1].sum(1)
        return y.mean(), y.var(ddof=1) / a.B
    return a.tot[f0:f1].sum(), a.tot_cov[f0:f1, f0:f1].sum()


def compare(a, ref, groups):
    """the rule of tests/test_gpu_sensors._agrees applied to cells: at most 1 + 1 % of the tested cells beyond 4 sigma of the combined variance, and
    every tested frame total within 4 sigma.  groups: tested(the right reference); ref: the Film to compare with; a: a Film or Batches.
    -> (agrees, outliers, tested, largest |z| of a cell, largest |z| of a frame total)"""
    cells, pools = groups
    z = np.empty(len(cells))
    for i, (b, f0, f1) in enumerate(cells):
        ma, va = _group(a, b, f0, f1); mr, vr = _group(ref, b, f0, f1)
        z[i] = (ma - mr) / np.sqrt(va + vr + 1e-14)
    zt = []
    for f0, f1 in pools:
        ma, va = _total(a, f0, f1); mr, vr = _total(ref, f0, f1)
        zt.append((ma - mr) / np.sqrt(va + vr + 1e-14))
    zt = np.array(zt)
    out = int((np.abs(z) > 4).sum())
    ok = out <= 1 + 0.01 * len(z) and bool(np.all(np.abs(zt) <= 4))
    print("   outliers %d of %d cells, max |z| %.2f; %d frame totals: max |z| %.2f; film %.5f vs %.5f" % (out, len(z), np.abs(z).max(), len(zt), np.abs(zt).max(), _totals(a)[0].sum(), ref.tot.sum()))
    return ok, out, len(z), float(np.abs(z).max()), float(np.abs(zt).max())


def agrees(a, ref, groups):
    return compare(a, ref, groups)[0]


def agrees_per_pixel(a, b):
    """tests/test_gpu_sensors._agrees on the frame-summed film: the one frame of a modulated film"""
    (ma, va), (mb, vb) = per_pixel(a), per_pixel(b)
    z = (ma - mb) / np.sqrt(va + vb + 1e-14)
    total = abs(ma.sum() - mb.sum()) <= 4 * np.sqrt(va.sum() + vb.sum())
    out = int((np.abs(z) > 4).sum())
    print("   outliers %d of %d pixels, max |z| %.2f, total %.5f vs %.5f" % (out, z.size, np.abs(z).max(), ma.sum(), mb.sum()))
    return out <= 1 + 0.01 * z.size and bool(total), out, float(np.abs(z).max())


def nontrivial_frames(ref):
    """the number of frames that each hold more than 2 % of the film's total"""
    return int((ref.tot > 0.02 * ref.tot.sum()).sum())


# ------------------------------------------------------------------------------------------------ single-scatter quadratures

PENCIL_O, PENCIL_D, PENCIL_T0, PENCIL_T1 = np.array([-3.0, 0.0, 0.0]), np.array([1.0, 0.0, 0.0]), 2.0, 4.0     # the central ray and its part in the cube


def _bin(length, f, frames):
    lo, bw, F = frames
    b = np.floor((np.ravel(length) - lo) / bw)
    m = (b >= 0) & (b < F)
    return np.bincount(b[m].astype(np.int64), weights=np.ravel(f)[m], minlength=F)


def _bin_span(la, lb, f, frames):
    """_bin for contributions whose length runs from la to lb across their depth cell: each spread evenly over its span.  It makes the binned
    midpoint rule second order in the depth step"""
    lo, bw, F = frames
    a = (np.ravel(np.minimum(la, lb)) - lo) / bw; b = (np.ravel(np.maximum(la, lb)) - lo) / bw; f = np.ravel(f)
    b = np.maximum(b, a + 1e-12)
    ka = np.floor(a)
    out = np.zeros(F)
    for j in range(int((np.floor(b) - ka).max()) + 1):
        k = ka + j
        w = f * np.maximum(np.minimum(b, k + 1) - np.maximum(a, k), 0.0) / (b - a)      # the share of the span inside bin k
        m = (k >= 0) & (k < F) & (w != 0)
        out += np.bincount(k[m].astype(np.int64), weights=w[m], minlength=F)
    return out


def spot_profile(spot, sigma_a, sigma_s, frames, calibrated=False, n=200000):
    """a spot INSIDE the cube, isotropic phase function: the 1-D integral of ref64.point_single_scatter times the cone's falloff"""
    assert np.all(np.abs(spot.position) < 1)
    _, t, f, r = ref64.point_single_scatter(PENCIL_O, PENCIL_D, PENCIL_T0, PENCIL_T1, sigma_a, sigma_s, spot.position, spot.I, n=n)
    x = PENCIL_O[None] + t[:, None] * PENCIL_D[None]
    fall = spot.falloff((spot.position[None] - x) / r[:, None])
    return _bin(t + r - (PENCIL_T0 if calibrated else 0.0), f * fall, frames)


def _depths(n_t, sigma_a, sigma_s):
    t = PENCIL_T0 + (np.arange(n_t) + 0.5) / n_t * (PENCIL_T1 - PENCIL_T0)
    return t, sigma_s * np.exp(-(sigma_a + sigma_s) * (t - PENCIL_T0)) * (PENCIL_T1 - PENCIL_T0) / n_t


def _area_points(shape, n):
    """midpoints of an n x n grid over the emitter's area: positions, normals, area elements"""
    a = (np.arange(n) + 0.5) / n
    A, B = [q.ravel() for q in np.meshgrid(a, a, indexing="ij")]
    if isinstance(shape, vs.Sphere):
        z = 1 - 2 * A; ph = 2 * np.pi * B; rr = np.sqrt(1 - z * z)
        w = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
        return shape.c + shape.R * w, w * shape.sign, np.full(n * n, shape.area / (n * n))
    lu, lv = np.linalg.norm(shape.u), np.linalg.norm(shape.v)
    if shape.disk:
        ph = 2 * np.pi * B
        q = shape.o + (A * np.cos(ph))[:, None] * shape.u + (A * np.sin(ph))[:, None] * shape.v
        dA = lu * lv * A * (2 * np.pi / (n * n))
    else:
        q = shape.o + (2 * A - 1)[:, None] * shape.u + (2 * B - 1)[:, None] * shape.v
        dA = np.full(n * n, 4 * lu * lv / (n * n))
    return q, np.broadcast_to(shape.n, q.shape), dA


def shape_profile(shape, sigma_a, sigma_s, g, frames, calibrated=False, n_t=400, n_a=64):
    """one convex emitter shape clear of the cube: the integral over depth and emitter area of Le cos / r^2 x visibility (the emitting side
    faces the vertex) x the two transmittances x the phase function, binned by depth + distance"""
    shape = as_shape(shape)
    st = sigma_a + sigma_s
    t, ft = _depths(n_t, sigma_a, sigma_s)
    q, nq, dA = _area_points(shape, n_a)
    h = (PENCIL_T1 - PENCIL_T0) / n_t
    out = np.zeros(frames[2])
    for t0 in range(0, n_t, 16):
        tt = t[t0:t0 + 16]
        x = PENCIL_O[None] + tt[:, None] * PENCIL_D[None]
        dv = q[None] - x[:, None]                                               # [t, a, 3]
        r = np.linalg.norm(dv, axis=2); w = dv / r[..., None]
        c = -np.sum(w * nq[None], 2)
        te = vm._exit(np.repeat(x, len(q), 0), w.reshape(-1, 3)).reshape(r.shape)
        f = ft[t0:t0 + 16, None] * shape.L * np.maximum(c, 0.0) / (r * r) * dA[None] * np.exp(-st * te) * ref64.hg_pdf(g, w @ PENCIL_D)
        ends = [(tt + s * h)[:, None] + np.linalg.norm(dv - (s * h) * PENCIL_D, axis=2) - (PENCIL_T0 if calibrated else 0.0) for s in (-0.5, 0.0, 0.5)]
        out += _bin_span(ends[0], ends[1], 0.5 * f, frames) + _bin_span(ends[1], ends[2], 0.5 * f, frames)
    return out


def map_profile(env, sigma_a, sigma_s, g, frames, calibrated=False, m=16, channel=0):
    """an environment map: the integral over depth and direction of Le x the transmittance to the cube's exit x the phase function, binned by
    depth + distance to the exit.  Directions: m x m midpoints per texel of the map's own lat-long grid (the bilinear interpolant's kinks lie on
    cell borders).  Depth: in closed form.  From the point (s, 0, 0) of the axis the exit lies at min((sign(wx) - s) / wx, 1 / |wy|, 1 / |wz|):
    along the depth the length t + exit is linear on either side of the one depth at which the exit face changes, and the integrand is the
    exponential of a linear function there, so a piece's share of a frame is an elementary integral"""
    st = sigma_a + sigma_s
    lo, bw, F = frames
    nth, nph = env.h * m, env.w * m
    th = (np.arange(nth) + 0.5) * np.pi / nth; ph = (np.arange(nph) + 0.5) * 2 * np.pi / nph
    TH, PH = [q.ravel() for q in np.meshgrid(th, ph, indexing="ij")]
    local = np.stack([np.sin(PH) * np.sin(TH), np.cos(TH), -np.cos(PH) * np.sin(TH)], 1)
    w = local @ env.R.T
    fw = sigma_s * env.eval(w)[0][:, channel] * np.sin(TH) * (np.pi / nth) * (2 * np.pi / nph) * ref64.hg_pdf(g, w @ PENCIL_D)
    with np.errstate(divide="ignore"):
        c = np.minimum(1 / np.abs(w[:, 1]), 1 / np.abs(w[:, 2]))                # the side faces: the same from every point of the axis
        wx = w[:, 0]
        # with t the depth from the camera (s = t - 3): the x face lies at (4 - t) / wx ahead (wx > 0) or (t - 2) / |wx| behind (wx < 0)
        tsw = np.clip(np.where(wx > 0, PENCIL_T1 - c * wx, PENCIL_T0 - c * wx), PENCIL_T0, PENCIL_T1)     # where the exit face changes
        a_x = np.where(wx > 0, PENCIL_T1 / wx, PENCIL_T0 / wx); b_x = -1 / wx      # exit through the x face = a_x + b_x t
    edges = lo + bw * np.arange(F + 1) + (PENCIL_T0 if calibrated else 0.0)
    out = np.zeros(F)
    side_first = wx > 0                                                         # wx > 0: the side face up to tsw, then the x face; wx < 0: the reverse
    for first in (True, False):
        on_side = side_first == first
        ta = np.where(first, PENCIL_T0, tsw); tb = np.where(first, tsw, PENCIL_T1)
        e0 = np.where(on_side, c, a_x); e1 = np.where(on_side, 0.0, b_x)        # exit = e0 + e1 t on this piece; length = e0 + (1 + e1) t
        q = -st * (1 + e1); p = -st * (e0 - PENCIL_T0)                            # the integrand: fw exp(p + q t)
        beta = 1 + e1
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            te = (edges[None, :] - e0[:, None]) / beta[:, None]                 # the depth at which the length reaches each frame edge
        te = np.clip(np.where(np.isfinite(te), te, 0.0), ta[:, None], tb[:, None])
        lo_t = np.where(beta[:, None] > 0, ta[:, None], te); hi_t = np.where(beta[:, None] > 0, te, tb[:, None])      # the depths whose length lies below the edge
        d = q[:, None] * (hi_t - lo_t)
        with np.errstate(divide="ignore", invalid="ignore"):
            ratio = np.where(np.abs(d) > 1e-8, np.expm1(d) / d, 1.0 + 0.5 * d)
        C = fw[:, None] * np.exp(p[:, None] + q[:, None] * lo_t) * (hi_t - lo_t) * ratio
        out += (C[:, 1:] - C[:, :-1]).sum(0)
    return out


def refined(profile, **steps):
    """profile(**steps) and the same at half the step in every dimension: (the finer profile, the largest relative change of a frame total among
    the frames that hold at least 1 % of the largest frame, the largest ABSOLUTE change among the fainter frames as a fraction of that 1 %).
    The fainter frames are those the support's edge grazes: the edge moves with the step, so their own totals converge slowly, and the z-tests
    pool them (pooled_frames)"""
    a = profile(**steps)
    b = profile(**{k: 2 * v for k, v in steps.items()})
    floor = 0.01 * b.max()
    main = b >= floor
    return b, float((np.abs(b - a)[main] / b[main]).max()), float((np.abs(b - a)[~main] / floor).max()) if (~main).any() else 0.0


# ------------------------------------------------------------------------------------------------ the scenes of the decomposed-film tests
# (tests/test_transient64.py builds and checks the float64 films on the CPU; tests/test_gpu_transient_extra.py repeats the GPU side)

NO_ROULETTE = 1 << 20                                                           # rr_depth: the float64 walks play no Russian roulette
SINGLE_MEDIUM = (0.3, 0.9)                                                      # sigma_a, sigma_s of closed_form.single_scatter_scene
SINGLE_FRAMES = (2.0, 0.25, 32)                                                 # [2, 10): the camera edge of the pencil camera is 2 = 8 frames
SINGLE_NAMES = ["spot", "rectangle", "disk", "sphere", "flipped_sphere", "map"]
SINGLE_RECT = np.array([[0.9, 0, 0, 0.3], [0, 0, -1, 2.0], [0, -0.6, 0, 0.1]], np.float64)          # above the cube, faces down
_c, _s = np.cos(np.deg2rad(25.0)), np.sin(np.deg2rad(25.0))
SINGLE_DISK = np.array([[0.7 * _c, 0, 0.7 * _s, -0.2], [0.7 * _s, 0, -0.7 * _c, 2.1], [0, -0.7, 0, 0.3]], np.float64)   # tilted, faces the cube
SINGLE_BALL = ([0.3, 2.4, 0.2], 0.7)
SINGLE_DOME = ([0.1, -0.1, 0.2], 4.0)                                           # inward-facing, around cube and camera
SINGLE_SPOT = ([-0.8, 0.3, -0.1], [0.6, -0.1, 0.0])                             # inside the cube, aimed down the ray: the cone's edge crosses it near the entry


def single_case(name):
    """one emitter over the pencil camera -> dict(emitter: the SceneParams.emitters entry, g, max_depth: exactly one scattering vertex,
    ref: points / spots / shapes / env of `render`, profile(frames, calibrated, **steps): the quadrature, steps: its resolution)"""
    from mitsubaer_amd import params as P
    from tests import volpath64_spot as vsp
    from tests.envmap64 import rot
    sa, ss = SINGLE_MEDIUM
    ref = dict(points=[], spots=[], shapes=[], env=0.0)
    if name == "spot":
        tw = np.asarray(P.look_at(SINGLE_SPOT[0], SINGLE_SPOT[1], [0.2, 1.0, 0.1]), np.float64)
        spot = vsp.Spot(tw, 2.0, 60.0)
        return dict(emitter=P.spot_emitter(tw, [2.0] * 3, 60.0), g=0.0, max_depth=3, ref=dict(ref, spots=[spot]), steps=dict(n=100000),
                    profile=lambda frames, calibrated=False, **kw: spot_profile(spot, sa, ss, frames, calibrated, **kw))
    if name == "map":
        from tests.combined_scenes import sun_map, ROT
        env = EnvMap64(sun_map(), ROT)
        return dict(emitter=P.envmap_emitter(sun_map(), ROT), g=0.5, max_depth=4, ref=dict(ref, env=env), steps=dict(m=16),
                    profile=lambda frames, calibrated=False, **kw: map_profile(env, sa, ss, 0.5, frames, calibrated, **kw))
    if name == "rectangle":
        em, sh = P.area_emitter(SINGLE_RECT, [4.0] * 3), vs.Planar(SINGLE_RECT, 4.0, False)
    elif name == "disk":
        em, sh = P.disk_emitter(SINGLE_DISK, [4.0] * 3), vs.Planar(SINGLE_DISK, 4.0, True)
    elif name == "sphere":
        em, sh = P.sphere_emitter(*SINGLE_BALL, [4.0] * 3), vs.Sphere(*SINGLE_BALL, 4.0)
    else:
        em, sh = P.sphere_emitter(*SINGLE_DOME, [0.5] * 3, flip_normals=True), vs.Sphere(*SINGLE_DOME, 0.5, flip=True)
    return dict(emitter=em, g=0.5, max_depth=4, ref=dict(ref, shapes=[sh]), steps=dict(n_t=200, n_a=128),
                profile=lambda frames, calibrated=False, **kw: shape_profile(sh, sa, ss, 0.5, frames, calibrated, **kw))


def single_params(name, **kw):
    """the GPU scene of single_case(name): transient over SINGLE_FRAMES, emitters hidden, a black constant environment"""
    from mitsubaer_amd import params as P
    from tests import closed_form
    c = single_case(name)
    lo, bw, F = SINGLE_FRAMES
    base = dict(point_intensity=[0.0] * 3, emitters=[c["emitter"]], hide_emitters=True, phase=P.PHASE_HG if c["g"] else P.PHASE_ISOTROPIC, g=c["g"],
                max_depth=c["max_depth"], rr_depth=NO_ROULETTE, decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=lo, max_bound=lo + bw * F, bin_width=bw)
    base.update(kw)
    return closed_form.single_scatter_scene(**base)


def single_render(name, spp, seed, **kw):
    """the time-resolved volpath on single_case(name): a 2 x 2 film, one block"""
    from mitsubaer_amd import params as P
    c = single_case(name)
    sa, ss = SINGLE_MEDIUM
    args = dict(frames=SINGLE_FRAMES, max_depth=c["max_depth"], hide_emitters=True, spp=spp, seed=seed, chunk=4096)
    args.update(kw)
    return render(S.PERSPECTIVE, c["ref"]["points"], c["ref"]["spots"], c["ref"]["shapes"], c["ref"]["env"], ss, sa, c["g"], 2, 2, 0.02,
                  np.asarray(P.look_at([-3, 0, 0], [-2, 0, 0], [0, 1, 0]), np.float64), **args)


MULTI_NAMES = ["lens_map_spot_point_rect", "lens_two_rects_two_spots", "parallel_map_points", "mixed_shapes"]
LENS_NAMES = MULTI_NAMES[:2]                                                    # the camera edge depends on the aperture sample
MODULATED_NAMES = ["lens_map_spot_point_rect", "mixed_shapes"]
TRANSIENT_FRAMES = (0.0, 0.5, 32)                                               # [0, 16)
BOUNCE_FRAMES = (0.0, 1.0, 16)
BOUNCE_DEPTH = 8
MULTI_SPP = 2048
# the GPU's batches in the multiple-scattering tests: 32 of 1024.  A cell is tested when 2048 float64 paths, each sampling EVERY emitter at
# every vertex, resolve it to 25 %.  The renderer selects one emitter per kind and vertex and divides by the probability, so one of its paths
# has up to 1 / p_min (3.5 to 7 here) times the second moment, carried by rare, large contributions: in the faintest tested cells a batch of
# 64 paths usually holds none of them, and 32 such batches report a small mean WITH a small variance -- no variance to test on.  1024 paths a
# batch are 16 x the reference's paths in all, more than the 7 x that the selection costs
MULTI_BATCH = 1024
SHADE_AT, SHADE_HALF, SHADE_RADIANCE = 3.4, 1.15, 6.0                            # combined_scenes.SHADE: 2.1, 0.7, 0.5
MODULATION = dict(mod_lambda=2.3, mod_phase_deg=25.0, mod_P=8)


def multi_scene(name):
    """-> (the steady SceneParams of the GPU render, the scene arguments of `render`)"""
    from mitsubaer_amd import params as P
    if name == "mixed_shapes":
        from tests.combined_scenes import mixed_params
        m = vs.MIXED
        return mixed_params(), dict(kind=S.PERSPECTIVE, points=[], spots=[], shapes=vs.mixed_shapes(), env=m["env"], sigma_s=m["sigma_s"], sigma_a=m["sigma_a"], g=m["g"],
                                     width=m["width"], height=m["height"], fov_x_deg=m["fov_x_deg"], cam_to_world=np.asarray(P.look_at(*vs.MIXED_CAM), np.float64))
    from tests import combined_scenes as tc
    p, ref, _ = tc.scene(name)
    a = dict(ref)
    # two of the three scenes are lit almost wholly by the map, whose path lengths fill 6 frames and do not depend on where a connecting edge
    # starts.  Until the profile is non-trivial and "edge_from_exit" shows, on both sides: the shade of the first scene stands further out (it
    # still covers the sun) and is brighter -- its point emitter has to stay inside the cube beside an area emitter --, and the points of the third
    # are four times as bright
    if name == "lens_map_spot_point_rect":
        shade = tc.facing_rect(SHADE_AT * tc.sun_direction(tc.ROT), SHADE_HALF)
        a["rects"] = [vm.Rect(shade, SHADE_RADIANCE)]
        p = p.copy(emitters=[P.area_emitter(shade, [SHADE_RADIANCE] * 3, e["sampling_weight"]) if e["type"] == P.EMITTER_AREA else e for e in p.emitters])
    if name == "parallel_map_points":
        a["points"] = [(q, 4.0 * i) for q, i in a["points"]]
        p = p.copy(emitters=[P.point_emitter(e["position"], [4.0 * v for v in e["intensity"]], e["sampling_weight"]) if e["type"] == P.EMITTER_POINT else e for e in p.emitters])
    a["shapes"] = a.pop("rects")
    a["cam_to_world"] = np.asarray(a["cam_to_world"], np.float64)
    a.update(sigma_s=tc.MED64[0], sigma_a=tc.MED64[1], g=tc.MED64[2], width=16, height=16, fov_x_deg=50.0)
    return p, a


def decomposed(p, what, **kw):
    """the GPU scene p with the film `what`: "transient" | "calibrated" | "bounce" | "sine" | "square" """
    from mitsubaer_amd import params as P
    lo, bw, F = BOUNCE_FRAMES if what == "bounce" else TRANSIENT_FRAMES
    q = dict(rr_depth=NO_ROULETTE, decomposition=P.DECOMPOSITION_BOUNCE if what == "bounce" else P.DECOMPOSITION_TRANSIENT, min_bound=lo, max_bound=lo + bw * F, bin_width=bw)
    if what == "bounce":
        q.update(max_depth=BOUNCE_DEPTH)
    if what == "calibrated":
        q.update(calibrated_transient=True)
    if what in ("sine", "square"):
        q.update(modulation=P.MODULATION_SINE if what == "sine" else P.MODULATION_SQUARE, **MODULATION)
    q.update(kw)
    return p.copy(**q)


@functools.lru_cache(maxsize=None)
def multi_reference(name):
    """every float64 film the tests need of one scene, binned from ONE walk of MULTI_SPP paths per pixel: {"transient", "transient/edge_from_exit",
    "bounce", "bounce/bounce_counts_exit"}, for the lens scenes {"calibrated"} (its wrong film, "calibrated_ignored", IS "transient"), for the
    modulated scenes {"sine", "square"}.  Computed once and shared"""
    p, args = multi_scene(name)
    keys = ["transient", "transient/edge_from_exit", "bounce", "bounce/bounce_counts_exit"]
    specs = [Spec(TRANSIENT_FRAMES), Spec(TRANSIENT_FRAMES, wrong="edge_from_exit"), Spec(BOUNCE_FRAMES, "bounce", max_depth=BOUNCE_DEPTH),
             Spec(BOUNCE_FRAMES, "bounce", wrong="bounce_counts_exit", max_depth=BOUNCE_DEPTH)]
    if name in LENS_NAMES:
        keys.append("calibrated"); specs.append(Spec(TRANSIENT_FRAMES, calibrated=True))
    if name in MODULATED_NAMES:
        from oracle import orc
        orc.build()
        for what in ("sine", "square"):
            keys.append(what); specs.append(Spec(weight=lambda l, q=decomposed(p, what): orc.correlation(q, l)))
    return dict(zip(keys, render(films=specs, spp=MULTI_SPP, seed=1, **args)))


@functools.lru_cache(maxsize=None)
def single_profile(name):
    """the quadrature of single_case(name) at the finer of the two resolutions tests/test_transient64.py compares, over SINGLE_FRAMES and 8 more
    frames: [:F] is the plain profile, [8:] the calibrated one (the camera edge is 2).  One cell = the 4 pixels: times 4.  Computed once"""
    c = single_case(name)
    lo, bw, F = SINGLE_FRAMES
    prof = 4 * c["profile"]((lo, bw, F + 8), **{k: 2 * v for k, v in c["steps"].items()})
    prof.setflags(write=False)
    return prof


def pooled_frames(prof, share=0.01):
    """frames of a profile pooled with the next until a pool holds `share` of the profile's total (what is left at the end joins the last
    pool): a z-test on a variance estimated from the samples themselves needs samples -- a frame that the support's edge merely grazes has
    none in most renders.  -> [(first, one past the last)]"""
    pools = []; f0 = 0
    for f in range(len(prof)):
        if prof[f0:f + 1].sum() >= share * prof.sum():
            pools.append((f0, f + 1)); f0 = f + 1
    if f0 < len(prof) and pools:
        pools[-1] = (pools[-1][0], len(prof))
    return pools


def resolved_frames(prof, share=0.01):
    """the number of frames that each hold `share` of the profile on their own: pooled_frames must leave about as many pools"""
    return int((prof >= share * prof.sum()).sum())


def profile_z(tot, tot_cov, prof):
    """z of every pool of pooled_frames(prof): tot, tot_cov the frame totals under test and the covariance of their means"""
    return np.array([(tot[a:b].sum() - prof[a:b].sum()) / np.sqrt(tot_cov[a:b, a:b].sum() + 1e-20) for a, b in pooled_frames(prof)])
