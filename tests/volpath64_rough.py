"""An independent vectorised float64 volpath for one tiny scene with a rough dielectric boundary (the estimator of DESIGN.md section 1,
"Rough dielectric boundary"): a homogeneous grey medium (isotropic phase, constant index eta) in the cube [-1, 1]^3 seen by a pinhole camera
outside it, straight rays, a constant environment and a point emitter outside the cube.

Per path: the camera ray meets the cube or sees the environment.  Every vertex below max_depth is processed and raises the depth by one:
  - a surface vertex (from outside or inside) samples the point emitter -- T I / r^2 eval(wi, wo) when it lies on the exterior side of the
    face (the cube is convex: no other shadowing), a vacuum edge of length r -- then samples the BSDF; a direction to the exterior collects
    the environment (weight 1), one to the interior starts a free flight;
  - a medium vertex multiplies by the albedo and samples the phase function (no emitter sampling: the shadow ray stops at the surface).
Optical path lengths (the transient film): the camera edge in vacuum, eta x the length inside, the emitter edge in vacuum.
The BSDF is tests/microfacet64.py; rays, free flights, the cube and the bookkeeping are written here.  Numbers come from numpy's generator:
only expectations are compared with the HIP path."""
import numpy as np
from tests import microfacet64 as mf, ref64


def _frame(n):
    """any orthonormal tangent pair of the unit normals n (n, 3): the BSDF is isotropic, so only its z axis matters"""
    a = np.where(np.abs(n[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    s = np.cross(a, n); s /= np.linalg.norm(s, axis=1, keepdims=True)
    return s, np.cross(n, s)


def _to_local(v, s, t, n):
    return np.stack([np.sum(v * s, 1), np.sum(v * t, 1), np.sum(v * n, 1)], 1)


def _slabs(o, d):
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (-1 - o) / d; t2 = (1 - o) / d
    return np.max(np.minimum(t1, t2), 1), np.min(np.maximum(t1, t2), 1)


def _face_normal(x):
    k = np.argmax(np.abs(x), 1)
    n = np.zeros_like(x); n[np.arange(len(x)), k] = np.sign(x[np.arange(len(x)), k])
    return n


def render(distr, eta=1.5, sigma_s=1.0, sigma_a=0.1, env=0.2, point=(-1.6, 1.4, 0.4), intensity=3.0, max_depth=6, width=16, height=16,
           fov_x_deg=50.0, cam_to_world=None, spp=4096, seed=0, frames=None, chunk=256):
    """per-pixel mean and variance of the per-path radiance (height, width); with frames = (min_bound, bin_width, count) also the image total
    of every transient frame and its variance (over sample indices)"""
    rng = np.random.default_rng(seed)
    pe = np.asarray(point, np.float64)
    npx = width * height
    s1 = np.zeros(npx); s2 = np.zeros(npx)
    ftot = [] if frames else None
    for c0 in range(0, spp, chunk):
        k = min(chunk, spp - c0)
        pix = np.tile(np.arange(npx), k)
        pos = np.stack([pix % width, pix // width], 1) + rng.random((len(pix), 2))
        o, d = ref64.pinhole_rays(cam_to_world, width, height, fov_x_deg, pos)
        N = len(pix)
        L = np.zeros(N)
        fr = np.zeros((N, frames[2])) if frames else None

        def add(idx, value, plen):
            np.add.at(L, idx, value)
            if frames:
                b = np.floor((plen - frames[0]) / frames[1])
                ok = (b >= 0) & (b < frames[2]) & (value != 0)
                np.add.at(fr, (idx[ok], b[ok].astype(int)), value[ok])

        tn, tf = _slabs(o, d)
        hit = (tn <= tf) & (tf > 0)
        add(np.where(~hit)[0], np.full((~hit).sum(), env), np.zeros((~hit).sum()))
        idx = np.where(hit)[0]
        x = o[idx] + d[idx] * tn[idx, None]; dirn = d[idx]; T = np.ones(len(idx)); plen = tn[idx].copy()
        depth = 1
        surface = np.ones(len(idx), bool)         # True: the vertex is on the surface, False: in the medium
        while len(idx) and depth < max_depth:
            # ---- surface vertices
            sv = surface
            if sv.any():
                xs = x[sv]; n = _face_normal(xs); s, t = _frame(n)
                wi = _to_local(-dirn[sv], s, t, n)
                de = pe - xs; r = np.linalg.norm(de, axis=1); de /= r[:, None]
                wl = _to_local(de, s, t, n)
                val, _ = mf.eval_pdf(distr, eta, wi, wl)
                le = np.where(wl[:, 2] > 0, T[sv] * intensity * val / (r * r), 0.0)
                add(idx[sv], le, plen[sv] + r)
                wo, w, _, _ = mf.sample(distr, eta, wi, rng.random((len(wi), 3)))
                Ts = T[sv] * w
                out = (w > 0) & (wo[:, 2] > 0)
                add(idx[sv][out], Ts[out] * env, plen[sv][out])
                T[sv] = Ts
                dw = s * wo[:, :1] + t * wo[:, 1:2] + n * wo[:, 2:3]
                dirn[sv] = dw
                alive_s = (w > 0) & (wo[:, 2] < 0)
                keep = np.ones(len(idx), bool); keep[np.where(sv)[0][~alive_s]] = False
            else:
                keep = np.ones(len(idx), bool)
            # ---- medium vertices (surface False): albedo and an isotropic phase sample
            mv = ~surface
            if mv.any():
                T[mv] *= sigma_s / (sigma_s + sigma_a)
                z = 1 - 2 * rng.random(mv.sum()); ph = 2 * np.pi * rng.random(mv.sum()); rr = np.sqrt(1 - z * z)
                dirn[mv] = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
            idx, x, dirn, T, plen = idx[keep], x[keep], dirn[keep], T[keep], plen[keep]
            depth += 1
            # ---- free flight inside the cube to the next vertex
            _, texit = _slabs(x, dirn)
            texit = np.maximum(texit, 0.0)
            tfl = -np.log1p(-rng.random(len(idx))) / (sigma_s + sigma_a)
            scat = tfl < texit
            step = np.where(scat, tfl, texit)
            x = x + dirn * step[:, None]; plen = plen + eta * step
            surface = ~scat
        s1 += np.bincount(pix, L, npx); s2 += np.bincount(pix, L * L, npx)
        if frames:
            ftot.append(fr.reshape(k, npx, frames[2]).sum(1))         # rows j * npx ... are sample j of every pixel
    mean = s1 / spp; var = s2 / spp - mean ** 2
    res = (mean.reshape(height, width), var.reshape(height, width))
    if frames:
        ft = np.concatenate(ftot)
        res = res + (ft.mean(0), ft.var(0) / spp)
    return res
