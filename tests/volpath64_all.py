"""One float64 volpath for everything the single-feature ones (tests/volpath64_multi.py, _spot.py, _envmap.py, _sensor.py) cover, at once: a
homogeneous grey medium with a Henyey-Greenstein phase function in the index-matched cube [-1, 1]^3, straight rays, no depth limit and no
Russian roulette; primary rays of any of the four sensors (tests/sensors64.py); point emitters, spot emitters (volpath64_spot.Spot),
one-sided rectangles (volpath64_multi.Rect) and an environment that is a constant or a map (envmap64.EnvMap64).  RGB radiance: the map is
coloured, everything else grey.

Per path: the primary ray sees the nearest rectangle (front: its radiance, back: nothing) or the environment along its direction, or it
enters the cube.  A free flight ends at a scattering vertex (weight x albedo) or leaves the cube, where an UNSCATTERED path collects what
the ray meets outside.  At every vertex x with propagation direction d:
  - every point and every spot (ALL of them: the GPU selects one of their common table by samplingWeight and divides by the probability;
    the expectation is the sum): I falloff / r^2 Tr(in-cube part of r) phase;
  - the environment's luminaire sample -- a uniform direction for the constant, sampleDirect for the map -- with the power heuristic against
    the phase pdf, BLOCKED when any rectangle lies along its direction (include/mer.h, n_emitters: "any one blocks the environment's
    luminaire sample");
  - every rectangle: a uniform point, its solid-angle pdf, blocked by every other rectangle in front of it, power heuristic against the
    phase pdf;
  - the phase sample wo: Tr(exit) x what the ray meets outside -- the NEAREST rectangle's radiance, or the environment along wo -- weighted
    against the pdf of the strategy that could have produced it: that rectangle's solid-angle pdf, or the environment's (pdfDirect of the
    map, 1 / 4 pi of the constant) ("the nearest one ends a ... look-up").
`env_sample_sees_rects = False` drops the blocking of the environment's luminaire sample: the estimator a renderer would implement that
tests its envmap samples against the medium only.  The GPU tests use it as the wrong reference their scene must tell apart."""
import numpy as np
from tests import ref64, sensors64 as S, volpath64_multi as vm
from tests.envmap64 import EnvMap64


def _env_eval(env, d):
    """(radiance (n, 3), solid-angle pdf of the environment's luminaire sample (n,)) along unit directions d"""
    if isinstance(env, EnvMap64):
        return env.eval(d)
    return np.full((len(d), 3), float(env)), np.full(len(d), vm.INV_FOURPI)


def _outside(rects, env, o, d, t0=0.0):
    """what a ray that has left the cube at o sees, RGB, and the pdf (from the point t0 behind o) of the strategy that samples it"""
    L, pdf = _env_eval(env, d)
    L = L.copy(); pdf = pdf.copy()
    tbest = np.full(len(o), np.inf)
    for r in rects:
        t = r.intersect(o, d)
        near = t < tbest
        c = d @ r.n
        tbest = np.where(near, t, tbest)
        L = np.where(near[:, None], np.where(c < 0, r.L, 0.0)[:, None], L)
        pdf = np.where(near, (t + t0) ** 2 / (r.area * np.maximum(np.abs(c), 1e-300)), pdf)
    return L, pdf


def render(kind, points, spots, rects, env, sigma_s, sigma_a, g, width, height, fov_x_deg, cam_to_world, aperture_radius=0.0, focus_distance=1.0,
           near=1e-2, far=1e4, spp=2048, seed=0, chunk=128, max_bounces=60, env_sample_sees_rects=True):
    """kind: sensors64 kind; points: [(position, intensity)]; spots: [Spot]; rects: [Rect]; env: a float or an EnvMap64.
    -> per-pixel mean and variance of the per-path radiance, (height, width, 3) each"""
    rng = np.random.default_rng(seed)
    st = sigma_s + sigma_a
    npx = width * height
    s1 = np.zeros((npx, 3)); s2 = np.zeros((npx, 3))
    is_map = isinstance(env, EnvMap64)
    lights = [(np.asarray(p, np.float64), float(i), None) for p, i in points] + [(s.position, s.I, s) for s in spots]
    for c0 in range(0, spp, chunk):
        k = min(chunk, spp - c0)
        pix = np.tile(np.arange(npx), k)
        N = len(pix)
        pos = np.stack([pix % width, pix // width], 1) + rng.random((N, 2))
        u = rng.random((N, 2)) if kind in (S.THINLENS, S.TELECENTRIC) else None
        o, d, _, _ = S.sensor_rays(kind, cam_to_world, width, height, fov_x_deg, near, far, pos, u, aperture_radius, focus_distance)
        L = np.zeros((N, 3))
        tn, tf = vm._slabs(o, d)
        cube = (tn <= tf) & (tf > 0)
        tcube = np.where(cube, np.maximum(tn, 0.0), np.inf)
        trect = np.full(N, np.inf)
        for r in rects:
            trect = np.minimum(trect, r.intersect(o, d))
        direct = ~(cube & (tcube <= trect))                                  # the ray ends on a rectangle or escapes
        L[direct] = _outside(rects, env, o[direct], d[direct])[0]
        idx = np.where(~direct)[0]
        x = o[idx] + d[idx] * tcube[idx, None]; dirn = d[idx]; T = np.ones(len(idx)); scattered = np.zeros(len(idx), bool)
        for _ in range(max_bounces + 1):
            if len(idx) == 0:
                break
            tex = vm._exit(x, dirn)
            tfl = -np.log1p(-rng.random(len(idx))) / st
            scat = tfl < tex
            lv = ~scat & ~scattered
            if lv.any():
                Lo, _ = _outside(rects, env, x[lv] + dirn[lv] * tex[lv, None], dirn[lv])
                np.add.at(L, idx[lv], T[lv, None] * Lo)
            idx, x, dirn, T = idx[scat], x[scat] + dirn[scat] * tfl[scat, None], dirn[scat], T[scat] * (sigma_s / st)
            scattered = np.ones(len(idx), bool)
            n = len(idx)
            if n == 0:
                break
            # points and spots: all of them
            for p, inten, spot in lights:
                dv = p - x; r = np.linalg.norm(dv, axis=1); dv /= r[:, None]
                fall = 1.0 if spot is None else spot.falloff(dv)
                f = ref64.hg_pdf(g, np.sum(dirn * dv, 1))
                np.add.at(L, idx, (T * inten * fall / (r * r) * np.exp(-st * np.minimum(r, vm._exit(x, dv))) * f)[:, None] * np.ones(3))
            # the environment's luminaire sample
            if is_map or env != 0:
                if is_map:
                    _, _, de, vop, epdf = env.sample(rng.random((n, 2)))
                else:
                    w = rng.random((n, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(1 - z * z)
                    de = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
                    epdf = np.full(n, vm.INV_FOURPI); vop = np.full((n, 3), float(env) / vm.INV_FOURPI)
                blocked = np.zeros(n, bool)
                if env_sample_sees_rects:
                    for r in rects:
                        blocked |= np.isfinite(r.intersect(x, de))
                f = ref64.hg_pdf(g, np.sum(dirn * de, 1))
                with np.errstate(divide="ignore", invalid="ignore"):
                    w = np.where((epdf > 0) & ~blocked, vm._mis(epdf, f), 0.0)
                np.add.at(L, idx, (T * np.exp(-st * vm._exit(x, de)) * f * w)[:, None] * vop)
            # rectangles: all of them, each blocked by the others in front of it
            for j, r in enumerate(rects):
                dv, dist, pdf, Le = r.sample(x, rng.random((n, 2)))
                blocked = np.zeros(n, bool)
                for i, q in enumerate(rects):
                    if i != j:
                        blocked |= q.intersect(x, dv) < dist
                f = ref64.hg_pdf(g, np.sum(dirn * dv, 1))
                np.add.at(L, idx, np.where(blocked, 0.0, T * Le / pdf * np.exp(-st * vm._exit(x, dv)) * f * vm._mis(pdf, f))[:, None] * np.ones(3))
            # the phase sample and the look-up along it
            wo = vm._hg_sample(g, dirn, rng.random((n, 2)))
            f = ref64.hg_pdf(g, np.sum(dirn * wo, 1))
            te = vm._exit(x, wo)
            Lo, epdf = _outside(rects, env, x + wo * te[:, None], wo, te)
            np.add.at(L, idx, (T * np.exp(-st * te) * vm._mis(f, epdf))[:, None] * Lo)
            dirn = wo
        for c in range(3):
            s1[:, c] += np.bincount(pix, L[:, c], npx); s2[:, c] += np.bincount(pix, L[:, c] ** 2, npx)
    mean = s1 / spp; var = s2 / spp - mean ** 2
    return mean.reshape(height, width, 3), var.reshape(height, width, 3)
