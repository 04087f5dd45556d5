"""An independent vectorised float64 volpath for one small scene with several emitters ("several point and area
emitters"): a homogeneous grey medium with a Henyey-Greenstein phase function in the index-matched cube [-1, 1]^3, straight rays, a constant
environment, point emitters (inside or outside the cube) and one-sided rectangles outside it that may hide one another.  No depth limit and no Russian
roulette: a path ends when it leaves the cube (or after `max_bounces` scatterings, whose remainder albedo^max_bounces is negligible).

Per path: the camera ray sees the nearest rectangle (front side: its radiance, back side: nothing) or the environment, or it enters the
cube.  A free flight then ends at a scattering vertex (weight x albedo) or leaves the cube, where the path collects what the ray meets
outside -- the nearest rectangle or the environment -- only if it has not scattered yet.  At every vertex x with propagation direction d:
  - every point emitter j: I_j / r^2 Tr(in-cube part of r) phase(d, dir) -- ALL of them (the GPU selects one with its samplingWeight; the expectation agrees);
  - the environment: a uniform direction, env Tr(exit) phase / (1 / 4 pi), blocked by any rectangle, power-heuristic weight against the phase pdf;
  - every rectangle k: a uniform point, its solid-angle pdf, one-sided radiance, Tr of the in-cube part, blocked by every other rectangle in
    front of it, power-heuristic weight against the phase pdf (again ALL rectangles, each with its own pdf, not a selection);
  - the phase sample wo: Tr(exit) x what the ray meets outside, weighted against the pdf of the strategy that could have produced it (the
    nearest rectangle's solid-angle pdf, or 1 / 4 pi for the environment); then the free flight along wo.
Numbers come from numpy's generator: only expectations are compared with the HIP path."""
import numpy as np
from tests import ref64

INV_FOURPI = 1.0 / (4.0 * np.pi)


class Rect:
    """the image of [-1,1]^2 x {0} under the 3x4 map M (columns u, v, normal, origin; u orthogonal to v); radiance into the half space of
    its normal u x v"""

    def __init__(self, M, radiance):
        M = np.asarray(M, np.float64)
        self.u, self.v, self.o = M[:, 0], M[:, 1], M[:, 3]
        n = np.cross(self.u, self.v)
        self.n = n / np.linalg.norm(n)
        if np.dot(self.n, M[:, 2]) < 0:
            self.n = -self.n
        self.area = 4 * np.linalg.norm(self.u) * np.linalg.norm(self.v)
        self.L = float(radiance)

    def intersect(self, o, d):
        """t > 0 of o + t d on the rectangle, else inf"""
        dn = d @ self.n
        with np.errstate(divide="ignore", invalid="ignore"):
            t = ((self.o - o) @ self.n) / dn
        q = o + d * t[:, None] - self.o
        a = (q @ self.u) / np.dot(self.u, self.u); b = (q @ self.v) / np.dot(self.v, self.v)
        ok = np.isfinite(t) & (t > 1e-9) & (np.abs(a) <= 1) & (np.abs(b) <= 1)
        return np.where(ok, t, np.inf)

    def sample(self, x, u2):
        """direction, distance, solid-angle pdf, radiance seen along the direction (0 from the back side)"""
        q = self.o + (2 * u2[:, :1] - 1) * self.u + (2 * u2[:, 1:] - 1) * self.v
        dv = q - x; dist = np.linalg.norm(dv, axis=1); dv /= dist[:, None]
        c = dv @ self.n
        pdf = dist * dist / (self.area * np.maximum(np.abs(c), 1e-300))
        return dv, dist, pdf, np.where(c < 0, self.L, 0.0)


def _slabs(o, d):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (-1 - o) / d; t2 = (1 - o) / d
    return np.max(np.minimum(t1, t2), 1), np.min(np.maximum(t1, t2), 1)


def _exit(x, d):
    return np.maximum(_slabs(x, d)[1], 0.0)


def _hg_sample(g, d, u2):
    mu = ref64.hg_inverse_cdf(g, u2[:, 0]) if g != 0 else 1 - 2 * u2[:, 0]
    a = np.where(np.abs(d[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    s = np.cross(a, d); s /= np.linalg.norm(s, axis=1, keepdims=True); t = np.cross(d, s)
    sn = np.sqrt(np.maximum(1 - mu * mu, 0)); ph = 2 * np.pi * u2[:, 1]
    return s * (sn * np.cos(ph))[:, None] + t * (sn * np.sin(ph))[:, None] + d * mu[:, None]


def _mis(a, b):
    return a * a / (a * a + b * b)


def _outside(rects, env, o, d, t0=0.0):
    """what a ray that has left the cube at o sees: (radiance, solid-angle pdf, from the point t0 behind o, of the strategy that samples it)"""
    tbest = np.full(len(o), np.inf); L = np.full(len(o), float(env)); pdf = np.full(len(o), INV_FOURPI)
    for r in rects:
        t = r.intersect(o, d)
        near = t < tbest
        c = d @ r.n
        tbest = np.where(near, t, tbest)
        L = np.where(near, np.where(c < 0, r.L, 0.0), L)
        pdf = np.where(near, (t + t0) ** 2 / (r.area * np.maximum(np.abs(c), 1e-300)), pdf)
    return L, pdf


def render(points, rects, env, sigma_s, sigma_a, g, width, height, fov_x_deg, cam_to_world, spp=4096, seed=0, chunk=128, max_bounces=60):
    """points: [(position, intensity)], rects: [Rect]; per-pixel mean and variance of the per-path radiance (height, width)"""
    rng = np.random.default_rng(seed)
    st = sigma_s + sigma_a
    npx = width * height
    s1 = np.zeros(npx); s2 = np.zeros(npx)
    for c0 in range(0, spp, chunk):
        k = min(chunk, spp - c0)
        pix = np.tile(np.arange(npx), k)
        pos = np.stack([pix % width, pix // width], 1) + rng.random((len(pix), 2))
        o, d = ref64.pinhole_rays(cam_to_world, width, height, fov_x_deg, pos)
        N = len(pix)
        L = np.zeros(N)
        tn, tf = _slabs(o, d)
        cube = (tn <= tf) & (tf > 0)
        tcube = np.where(cube, np.maximum(tn, 0.0), np.inf)
        # the nearest rectangle in front of the cube (or instead of it)
        trect = np.full(N, np.inf); Lrect = np.zeros(N)
        for r in rects:
            t = r.intersect(o, d); near = t < trect
            trect = np.where(near, t, trect); Lrect = np.where(near, np.where(d @ r.n < 0, r.L, 0.0), Lrect)
        first_rect = trect < tcube
        L[first_rect] = Lrect[first_rect]
        miss = ~cube & ~first_rect
        L[miss] = env
        idx = np.where(cube & ~first_rect)[0]
        x = o[idx] + d[idx] * tcube[idx, None]; dirn = d[idx]; T = np.ones(len(idx)); scattered = np.zeros(len(idx), bool)
        for _ in range(max_bounces + 1):
            if len(idx) == 0:
                break
            tex = _exit(x, dirn)
            tfl = -np.log1p(-rng.random(len(idx))) / st
            scat = tfl < tex
            # leaving the cube: emission only on the unscattered camera path
            lv = ~scat
            if lv.any():
                xo = x[lv] + dirn[lv] * tex[lv, None]
                Lo, _ = _outside(rects, env, xo, dirn[lv])
                np.add.at(L, idx[lv], np.where(scattered[lv], 0.0, T[lv] * Lo))
            idx, x, dirn, T = idx[scat], x[scat] + dirn[scat] * tfl[scat, None], dirn[scat], T[scat] * (sigma_s / st)
            scattered = np.ones(len(idx), bool)
            n = len(idx)
            if n == 0:
                break
            # point emitters: all of them
            for p, inten in points:
                dv = np.asarray(p, np.float64) - x; r = np.linalg.norm(dv, axis=1); dv /= r[:, None]
                f = ref64.hg_pdf(g, np.sum(dirn * dv, 1))
                np.add.at(L, idx, T * inten / (r * r) * np.exp(-st * np.minimum(r, _exit(x, dv))) * f)     # outside the cube: its in-cube part
            # environment
            if env != 0:
                w = rng.random((n, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(1 - z * z)
                de = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
                te = _exit(x, de)
                blocked = np.zeros(n, bool)
                for r in rects:
                    blocked |= np.isfinite(r.intersect(x, de))
                f = ref64.hg_pdf(g, np.sum(dirn * de, 1))
                np.add.at(L, idx, np.where(blocked, 0.0, T * env / INV_FOURPI * np.exp(-st * te) * f * _mis(INV_FOURPI, f)))
            # rectangles: all of them, each blocked by the others in front of it
            for k, r in enumerate(rects):
                dv, dist, pdf, Le = r.sample(x, rng.random((n, 2)))
                blocked = np.zeros(n, bool)
                for j, q in enumerate(rects):
                    if j != k:
                        blocked |= q.intersect(x, dv) < dist
                f = ref64.hg_pdf(g, np.sum(dirn * dv, 1))
                te = _exit(x, dv)
                np.add.at(L, idx, np.where(blocked, 0.0, T * Le / pdf * np.exp(-st * te) * f * _mis(pdf, f)))
            # phase sample and the emitter look-up along it
            wo = _hg_sample(g, dirn, rng.random((n, 2)))
            f = ref64.hg_pdf(g, np.sum(dirn * wo, 1))
            te = _exit(x, wo)
            Lo, epdf = _outside(rects, env, x + wo * te[:, None], wo, te)
            np.add.at(L, idx, T * np.exp(-st * te) * Lo * _mis(f, epdf))
            dirn = wo
        s1 += np.bincount(pix, L, npx); s2 += np.bincount(pix, L * L, npx)
    mean = s1 / spp; var = s2 / spp - mean ** 2
    return mean.reshape(height, width), var.reshape(height, width)
