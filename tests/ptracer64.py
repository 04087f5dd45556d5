"""An independent vectorised float64 light tracer (the estimator of include/mer.h: mer_scene_desc.integrator = ptracer) for one small family
of scenes: a grey homogeneous medium with a Henyey-Greenstein phase function in the index-matched cube [-1, 1]^3, straight rays, a pinhole, a
box filter of radius 0.5 (a contribution lands in the pixel that contains its film position), and ONE emitter -- a point emitter or a
collimated beam.  Paths start at the emitter; every scattering vertex x with propagation direction d is connected to the pinhole:

    value = throughput x Phi x W(x) x p_HG(d . dir) x exp(-sigma_t l(x)),     W(x) = 1 / (A' cos^3 theta_c) / r^2,

with Phi = the beam's power (4 pi I for a point emitter), r the distance to the pinhole, l the in-cube part of that segment, theta_c the
angle to the optical axis and A' = (2 tan(fov_x / 2))^2 / aspect the image rectangle at depth 1 (PerspectiveCamera::importance).  The pixel
value is (1 / S) x the sum of the contributions of the W H S paths: the reference's setBitmap(accum, W H / particles).

Depths count as in ParticleTracer::process: the path starts at depth 1, the null boundary of the cube costs one depth for an emitter outside
it, a vertex found at depth k is connected when k < max_depth and the connection's one boundary crossing is allowed (max_depth - k - 1 != 0);
max_depth < 0: no limit.  No Russian roulette: a path ends when it leaves the cube (or after max_bounces scatterings).
Numbers come from numpy's generator: only expectations are compared with the HIP path.

single_scatter_quadrature is the closed form the tracer itself is pinned to: the once-scattered light of a collimated beam as a midpoint
rule over the beam, binned by pixel (and by path length for a transient film)."""
import numpy as np
from tests import ref64


def _slabs(o, d):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (-1 - o) / d; t2 = (1 - o) / d
    return np.max(np.minimum(t1, t2), -1), np.min(np.maximum(t1, t2), -1)


def _exit(x, d):
    return np.maximum(_slabs(x, d)[1], 0.0)


class Pinhole:
    def __init__(self, cam_to_world, width, height, fov_x_deg, near=1e-2, far=1e4):
        m = np.asarray(cam_to_world, np.float64)
        self.R, self.o = m[:3, :3], m[:3, 3]
        self.w, self.h = int(width), int(height)
        self.tan = np.tan(np.radians(fov_x_deg) / 2.0)
        self.aspect = width / float(height)
        self.area = (2.0 * self.tan) ** 2 / self.aspect
        self.near, self.far = near, far

    def connect(self, x):
        """(weight W(x) = importance / r^2 -- 0 outside the frustum or the clip range --, film position (n, 2) in pixels, unit direction to
        the pinhole, distance)"""
        v = x - self.o
        loc = v @ self.R                                            # R^T v, row-wise
        z = loc[:, 2]
        ok = (z >= self.near) & (z <= self.far)
        zs = np.where(ok, z, 1.0)
        u = 0.5 * (1.0 - loc[:, 0] / zs / self.tan); w = 0.5 * (1.0 - loc[:, 1] / zs * self.aspect / self.tan)
        ok &= (u >= 0) & (u <= 1) & (w >= 0) & (w <= 1)
        r = np.linalg.norm(v, axis=1)
        cos = np.where(ok, z / r, 1.0)
        W = np.where(ok, 1.0 / (self.area * cos ** 3) / (r * r), 0.0)
        return W, np.stack([u * self.w, w * self.h], 1), -v / r[:, None], r


def _hg_sample(g, d, u2):
    mu = ref64.hg_inverse_cdf(g, u2[:, 0]) if g != 0 else 1 - 2 * u2[:, 0]
    a = np.where(np.abs(d[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    s = np.cross(a, d); s /= np.linalg.norm(s, axis=1, keepdims=True); t = np.cross(d, s)
    sn = np.sqrt(np.maximum(1 - mu * mu, 0)); ph = 2 * np.pi * u2[:, 1]
    return s * (sn * np.cos(ph))[:, None] + t * (sn * np.sin(ph))[:, None] + d * mu[:, None]


def point(position, intensity):
    return {"kind": "point", "o": np.asarray(position, np.float64), "phi": 4.0 * np.pi * float(intensity)}


def collimated(origin, direction, power):
    d = np.asarray(direction, np.float64)
    return {"kind": "collimated", "o": np.asarray(origin, np.float64), "d": d / np.linalg.norm(d), "phi": float(power)}


def _frames(transient):
    return 1 if transient is None else int(np.ceil((transient[1] - transient[0]) / transient[2]))


def render(emitter, sigma_s, sigma_a, g, width, height, fov_x_deg, cam_to_world, spp=64, seed=0, max_depth=-1, transient=None, batches=16,
           max_bounces=60, full=False):
    """transient = (min_bound, max_bound, bin_width) bins every contribution by its path length (emitter -> vertices -> pinhole, index 1).
    The W H spp paths run as `batches` independent renders of spp / batches samples: returns (mean, variance of that mean), each
    (height, width, frames); full = True: the films of the batches instead, (batches, height, width, frames)."""
    assert spp % batches == 0
    rng = np.random.default_rng(seed)
    cam = Pinhole(cam_to_world, width, height, fov_x_deg)
    st = sigma_s + sigma_a
    F = _frames(transient)
    npx = width * height
    cam_inside = bool(np.all(np.abs(cam.o) <= 1))
    imgs = np.zeros((batches, npx * F))
    sb = spp // batches
    for b in range(batches):
        N = npx * sb
        if emitter["kind"] == "point":
            w = rng.random((N, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(np.maximum(1 - z * z, 0))
            d = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
        else:
            d = np.tile(emitter["d"], (N, 1))
        x = np.tile(emitter["o"], (N, 1))
        T = np.full(N, emitter["phi"]); plen = np.zeros(N)
        depth = 1
        if not np.all(np.abs(emitter["o"]) <= 1):                        # outside: to the null boundary, one depth
            tn, tf = _slabs(x, d)
            hit = (tn <= tf) & (tn > 0)
            x, d, T = x[hit] + d[hit] * tn[hit, None], d[hit], T[hit]; plen = tn[hit]
            depth = 2
        acc = np.zeros(npx * F)
        for _ in range(max_bounces):
            if len(T) == 0 or not (depth <= max_depth or max_depth < 0):
                break
            tex = _exit(x, d)
            tfl = -np.log1p(-rng.random(len(T))) / st
            sc = tfl < tex
            x, d, T, plen = x[sc] + d[sc] * tfl[sc, None], d[sc], T[sc] * (sigma_s / st), plen[sc] + tfl[sc]
            if len(T) == 0:
                break
            crossing_ok = cam_inside or (max_depth - depth - 1 != 0)
            if not (depth >= max_depth and max_depth > 0) and crossing_ok:
                W, uv, dv, r = cam.connect(x)
                val = T * W * ref64.hg_pdf(g, np.sum(d * dv, 1)) * np.exp(-st * np.minimum(r, _exit(x, dv)))
                px = np.minimum(uv[:, 0].astype(int), width - 1); py = np.minimum(uv[:, 1].astype(int), height - 1)
                idx = (py * width + px) * F
                keep = val > 0
                if transient is not None:
                    fb = np.floor((plen + r - transient[0]) / transient[2])
                    keep &= (fb >= 0) & (fb < F)
                    idx = idx + np.where(keep, fb, 0).astype(int)
                acc += np.bincount(idx[keep], val[keep], npx * F)
            d = _hg_sample(g, d, rng.random((len(T), 2)))
            depth += 1
        imgs[b] = acc / sb
    if full:
        return imgs.reshape(batches, height, width, F)
    mean = imgs.mean(0); var = imgs.var(0, ddof=1) / batches
    return mean.reshape(height, width, F), var.reshape(height, width, F)


def single_scatter_quadrature(beam, sigma_s, sigma_a, g, width, height, fov_x_deg, cam_to_world, transient=None, n=200000, rtol=1e-6):
    """Expected film of the ONCE-scattered light of a collimated beam:
        pixel p = W H Phi int sigma_s e^{-sigma_t s} p_HG(theta(s)) e^{-sigma_t l(s)} [1 / (A' cos^3 theta_c)] / r(s)^2 ds
    over the in-cube beam points that project into p (s = the in-cube beam length), by the midpoint rule with n nodes, n doubled until the
    film total changes by less than rtol.  transient = (min, max, bin width) restricts frame f to the nodes whose path length s_0 + s + r
    (s_0 = the beam's length in front of the cube) falls into it.  Returns (height, width, frames)."""
    cam = Pinhole(cam_to_world, width, height, fov_x_deg)
    st = sigma_s + sigma_a
    o, d = beam["o"], beam["d"]
    tn, tf = _slabs(o[None], d[None])
    t0, t1 = max(float(tn[0]), 0.0), float(tf[0])
    assert t1 > t0
    F = _frames(transient)

    def film(n):
        ds = (t1 - t0) / n
        s = (np.arange(n) + 0.5) * ds
        x = o + d * (t0 + s)[:, None]
        W, uv, dv, r = cam.connect(x)
        val = beam["phi"] * sigma_s * np.exp(-st * s) * ref64.hg_pdf(g, dv @ d) * np.exp(-st * np.minimum(r, _exit(x, dv))) * W * ds
        px = np.minimum(uv[:, 0].astype(int), width - 1); py = np.minimum(uv[:, 1].astype(int), height - 1)
        idx = (py * width + px) * F
        keep = val > 0
        if transient is not None:
            fb = np.floor((t0 + s + r - transient[0]) / transient[2])
            keep &= (fb >= 0) & (fb < F)
            idx = idx + np.where(keep, fb, 0).astype(int)
        return width * height * np.bincount(idx[keep], val[keep], width * height * F)

    prev = film(n)
    for _ in range(8):
        n *= 2
        cur = film(n)
        done = abs(cur.sum() - prev.sum()) <= rtol * abs(cur.sum())
        prev = cur
        if done:
            break
    else:
        raise AssertionError("single_scatter_quadrature did not converge")
    return prev.reshape(height, width, F)
