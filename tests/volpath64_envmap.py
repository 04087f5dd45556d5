"""The float64 volpath of tests/volpath64_spot.py lit by an environment map (src/emitters/envmap.cpp) instead of the constant environment:
a homogeneous grey medium with a Henyey-Greenstein phase function in the index-matched cube [-1, 1]^3, straight rays, RGB radiance.  No
depth limit and no Russian roulette.  Per path: a camera ray that misses the cube sees the map along its direction; a free flight that
leaves the cube before it has scattered sees the map along the same direction.  At every scattering vertex x with propagation direction d:
  - the luminaire sample: sampleDirect of the map (tests/envmap64.py: sampleReuse, tent offset, bilinear texels), value / pdf x Tr(exit)
    x phase, power-heuristic weight of its pdf against the phase pdf;
  - the phase sample wo: Tr(exit) x the map along wo, weighted with pdfDirect(wo) against the phase pdf; then the free flight along wo.
The map's value, pdf and sampler come from tests/envmap64.py, a float64 restatement of the reference written independently of the HIP code."""
import numpy as np
from tests import volpath64_multi as vm


def render(env, sigma_s, sigma_a, g, width, height, fov_x_deg, cam_to_world, spp=4096, seed=0, chunk=128, max_bounces=60):
    """env: tests.envmap64.EnvMap64; per-pixel mean and variance of the per-path RGB radiance (height, width, 3)"""
    rng = np.random.default_rng(seed)
    st = sigma_s + sigma_a
    npx = width * height
    s1 = np.zeros((npx, 3)); s2 = np.zeros((npx, 3))
    for c0 in range(0, spp, chunk):
        k = min(chunk, spp - c0)
        pix = np.tile(np.arange(npx), k)
        pos = np.stack([pix % width, pix // width], 1) + rng.random((len(pix), 2))
        o, d = vm.ref64.pinhole_rays(cam_to_world, width, height, fov_x_deg, pos)
        N = len(pix)
        L = np.zeros((N, 3))
        tn, tf = vm._slabs(o, d)
        cube = (tn <= tf) & (tf > 0)
        L[~cube] = env.eval(d[~cube])[0]
        idx = np.where(cube)[0]
        x = o[idx] + d[idx] * np.maximum(tn[idx], 0.0)[:, None]; dirn = d[idx]; T = np.ones(len(idx)); scattered = np.zeros(len(idx), bool)
        for _ in range(max_bounces + 1):
            if len(idx) == 0:
                break
            tex = vm._exit(x, dirn)
            tfl = -np.log1p(-rng.random(len(idx))) / st
            scat = tfl < tex
            lv = ~scat & ~scattered
            if lv.any():
                np.add.at(L, idx[lv], T[lv, None] * env.eval(dirn[lv])[0])
            idx, x, dirn, T = idx[scat], x[scat] + dirn[scat] * tfl[scat, None], dirn[scat], T[scat] * (sigma_s / st)
            scattered = np.ones(len(idx), bool)
            n = len(idx)
            if n == 0:
                break
            _, _, de, vop, epdf = env.sample(rng.random((n, 2)))
            f = vm.ref64.hg_pdf(g, np.sum(dirn * de, 1))
            with np.errstate(divide="ignore", invalid="ignore"):
                w = np.where(epdf > 0, vm._mis(epdf, f), 0.0)
            np.add.at(L, idx, (T * np.exp(-st * vm._exit(x, de)) * f * w)[:, None] * vop)
            wo = vm._hg_sample(g, dirn, rng.random((n, 2)))
            f = vm.ref64.hg_pdf(g, np.sum(dirn * wo, 1))
            val, pdf = env.eval(wo)
            np.add.at(L, idx, (T * np.exp(-st * vm._exit(x, wo)) * vm._mis(f, pdf))[:, None] * val)
            dirn = wo
        for c in range(3):
            s1[:, c] += np.bincount(pix, L[:, c], npx); s2[:, c] += np.bincount(pix, L[:, c] ** 2, npx)
    mean = s1 / spp; var = s2 / spp - mean ** 2
    return mean.reshape(height, width, 3), var.reshape(height, width, 3)
