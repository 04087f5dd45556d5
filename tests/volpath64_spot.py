"""The float64 volpath of tests/volpath64_multi.py with spot emitters (src/emitters/spot.cpp:66-200): a homogeneous grey medium with a
Henyey-Greenstein phase function in the index-matched cube [-1, 1]^3, straight rays, a constant environment, point emitters and spot
emitters.  No depth limit and no Russian roulette.  At every vertex x with propagation direction d it samples
  - every point emitter j: I_j / r^2 Tr(in-cube part of r) phase(d, dir);
  - every spot emitter j: the same, times falloffCurve(toWorld^-1 (-dir)) (spot.cpp:105-118, 184-199) -- ALL of them at every vertex (the
    GPU selects one point-table entry with its samplingWeight; the expectation agrees);
  - the environment: a uniform direction, power-heuristic weight against the phase pdf;
  - the phase sample wo: Tr(exit) x the environment, weighted against the uniform pdf; then the free flight along wo.
The falloff is written here from the reference's definition, in float64, independently of the HIP code."""
import numpy as np
from tests import volpath64_multi as vm


class Spot:
    """emitter `spot`: to_world (3x4 or 4x4), peak intensity (grey), cutoff / beam width in degrees (beam: 3/4 of the cutoff by default)"""

    def __init__(self, to_world, intensity, cutoff_deg=20.0, beam_deg=None):
        M = np.eye(4)
        t = np.asarray(to_world, np.float64)
        M[:t.shape[0], :4] = t
        self.position = M[:3, 3].copy()
        self.zrow = np.linalg.inv(M[:3, :3])[2]             # row 2 of the inverse linear part: cosTheta is NOT normalised
        self.cutoff = np.radians(float(cutoff_deg))
        self.beam = np.radians(float(cutoff_deg) * 0.75 if beam_deg is None else float(beam_deg))
        self.I = float(intensity)

    def falloff(self, d):
        """falloffCurve(trafo.inverse()(-d)) for unit directions d (n x 3) from the shading points to the emitter"""
        c = (-np.asarray(d, np.float64)) @ self.zrow
        with np.errstate(divide="ignore", invalid="ignore"):
            ramp = (self.cutoff - np.arccos(np.clip(c, -1.0, 1.0))) / (self.cutoff - self.beam)
        return np.where(c <= np.cos(self.cutoff), 0.0, np.where(c >= np.cos(self.beam), 1.0, ramp))

    def sample_direct(self, ref):
        """SpotEmitter::sampleDirect at the reference points (n x 3): value, unit direction to the emitter, distance, falloff"""
        dv = self.position - np.asarray(ref, np.float64)
        dist = np.linalg.norm(dv, axis=1)
        d = dv / dist[:, None]
        f = self.falloff(d)
        return self.I * f / (dist * dist), d, dist, f


def render(points, spots, env, sigma_s, sigma_a, g, width, height, fov_x_deg, cam_to_world, spp=4096, seed=0, chunk=128, max_bounces=60):
    """points: [(position, intensity)], spots: [Spot]; per-pixel mean and variance of the per-path radiance (height, width)"""
    rng = np.random.default_rng(seed)
    st = sigma_s + sigma_a
    npx = width * height
    s1 = np.zeros(npx); s2 = np.zeros(npx)
    lights = [(np.asarray(p, np.float64), float(i), None) for p, i in points] + [(s.position, s.I, s) for s in spots]
    for c0 in range(0, spp, chunk):
        k = min(chunk, spp - c0)
        pix = np.tile(np.arange(npx), k)
        pos = np.stack([pix % width, pix // width], 1) + rng.random((len(pix), 2))
        o, d = vm.ref64.pinhole_rays(cam_to_world, width, height, fov_x_deg, pos)
        N = len(pix)
        L = np.zeros(N)
        tn, tf = vm._slabs(o, d)
        cube = (tn <= tf) & (tf > 0)
        L[~cube] = env
        idx = np.where(cube)[0]
        x = o[idx] + d[idx] * np.maximum(tn[idx], 0.0)[:, None]; dirn = d[idx]; T = np.ones(len(idx)); scattered = np.zeros(len(idx), bool)
        for _ in range(max_bounces + 1):
            if len(idx) == 0:
                break
            tex = vm._exit(x, dirn)
            tfl = -np.log1p(-rng.random(len(idx))) / st
            scat = tfl < tex
            lv = ~scat
            np.add.at(L, idx[lv], np.where(scattered[lv], 0.0, T[lv] * env))
            idx, x, dirn, T = idx[scat], x[scat] + dirn[scat] * tfl[scat, None], dirn[scat], T[scat] * (sigma_s / st)
            scattered = np.ones(len(idx), bool)
            n = len(idx)
            if n == 0:
                break
            for p, inten, spot in lights:
                dv = p - x; r = np.linalg.norm(dv, axis=1); dv /= r[:, None]
                fall = 1.0 if spot is None else spot.falloff(dv)
                f = vm.ref64.hg_pdf(g, np.sum(dirn * dv, 1))
                np.add.at(L, idx, T * inten * fall / (r * r) * np.exp(-st * np.minimum(r, vm._exit(x, dv))) * f)
            if env != 0:
                w = rng.random((n, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(1 - z * z)
                de = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
                f = vm.ref64.hg_pdf(g, np.sum(dirn * de, 1))
                np.add.at(L, idx, T * env / vm.INV_FOURPI * np.exp(-st * vm._exit(x, de)) * f * vm._mis(vm.INV_FOURPI, f))
            wo = vm._hg_sample(g, dirn, rng.random((n, 2)))
            f = vm.ref64.hg_pdf(g, np.sum(dirn * wo, 1))
            np.add.at(L, idx, T * np.exp(-st * vm._exit(x, wo)) * env * vm._mis(f, vm.INV_FOURPI))
            dirn = wo
        s1 += np.bincount(pix, L, npx); s2 += np.bincount(pix, L * L, npx)
    mean = s1 / spp; var = s2 / spp - mean ** 2
    return mean.reshape(height, width), var.reshape(height, width)
