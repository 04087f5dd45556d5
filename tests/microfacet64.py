"""Float64 restatement of the rough dielectric boundary (hroughdielectric), numpy / scipy only, written from the published models:
Walter, Marschner, Li, Torrance 2007 (Beckmann, GGX and Phong distributions, Smith masking, the rough dielectric BSDF, half-vector
Jacobians) and Heitz, d'Eon 2014 (sampling of the visible normals).  Conventions (isotropic alpha >= 1e-4, the Phong exponent
2 / alpha^2 - 2, visible sampling off for Phong, Walter's sampling-alpha widening 1.2 - 0.2 sqrt|cos theta_i|, the lobe sampled around
sign(cos theta_i) wi, ERadiance (1/eta)^2 on refractions into the medium) are the reference's.  Vectors are (n, 3) arrays in the local
frame (z = the outward normal); eta = interior / exterior index.  Ground truth for tests/test_gpu_rough_dielectric.py; proven against
itself in tests/test_host_rough_dielectric.py."""
import numpy as np
from scipy import special, stats

BECKMANN, GGX, PHONG = 0, 1, 2


def frame(n):
    """Mitsuba's Frame(n): coordinateSystem (util.cpp:606-615) -> (s, t); local = (v.s, v.t, v.n)"""
    n = np.asarray(n, np.float64)
    if abs(n[0]) > abs(n[1]):
        c = np.array([n[2], 0.0, -n[0]]) / np.hypot(n[0], n[2])
    else:
        c = np.array([0.0, n[2], -n[1]]) / np.hypot(n[1], n[2])
    return np.cross(c, n), c


class Distr:
    def __init__(self, kind, alpha, visible=True):
        self.kind = kind
        self.alpha = max(float(alpha), 1e-4)
        self.visible = bool(visible) and kind != PHONG

    def scaled(self, s):
        """the same distribution with alpha x s (s may be an array: one alpha per item)"""
        d = Distr(self.kind, 1.0, self.visible)
        d.alpha = self.alpha * np.asarray(s, np.float64)
        return d

    @property
    def exponent(self):
        return np.maximum(2.0 / self.alpha ** 2 - 2.0, 0.0)

    def D(self, m):
        c = m[:, 2]
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            c2 = c * c
            t2a = (m[:, 0] ** 2 + m[:, 1] ** 2) / (c2 * self.alpha ** 2)
            if self.kind == GGX:
                r = (1 + t2a) * c2
                v = 1.0 / (np.pi * self.alpha ** 2 * r * r)
            elif self.kind == PHONG:
                v = (self.exponent + 2) / (2 * np.pi) * np.abs(c) ** self.exponent
            else:
                v = np.exp(-t2a) / (np.pi * self.alpha ** 2 * c2 * c2)
        return np.where(c > 0, v, 0.0)

    def G1(self, v, m):
        with np.errstate(divide="ignore", invalid="ignore"):
            tan = np.abs(np.sqrt(np.maximum(0.0, 1 - v[:, 2] ** 2)) / v[:, 2])
            if self.kind == GGX:
                r = self.alpha * tan
                g = 2.0 / (1 + np.sqrt(1 + r * r))
            else:
                a = 1.0 / (self.alpha * tan)
                g = np.where(a >= 1.6, 1.0, (3.535 * a + 2.181 * a * a) / (1 + 2.276 * a + 2.577 * a * a))
        g = np.where(tan == 0, 1.0, g)
        return np.where(np.sum(v * m, 1) * v[:, 2] <= 0, 0.0, g)

    def pdf_m(self, v, m):
        """density of the sampled normal: visible normals seen from v (v.z > 0), or D(m) cos theta_m"""
        if not self.visible:
            return self.D(m) * m[:, 2]
        with np.errstate(divide="ignore", invalid="ignore"):
            return np.where(v[:, 2] != 0, self.D(m) * self.G1(v, m) * np.abs(np.sum(v * m, 1)) / v[:, 2], 0.0)

    def sample_all(self, u1, u2):
        if self.kind == PHONG:
            c = u1 ** (1.0 / (self.exponent + 2))
        else:
            t2 = self.alpha ** 2 * (u1 / (1 - u1) if self.kind == GGX else -np.log1p(-u1))
            c = 1 / np.sqrt(1 + t2)
        s = np.sqrt(np.maximum(0.0, 1 - c * c)); phi = 2 * np.pi * u2
        return np.stack([s * np.cos(phi), s * np.sin(phi), c], 1)

    def sample_visible(self, v, u1, u2):
        a = self.alpha
        vs = np.stack([a * v[:, 0], a * v[:, 1], v[:, 2]], 1)
        vs /= np.linalg.norm(vs, axis=1, keepdims=True)
        st = np.sqrt(np.maximum(0.0, 1 - vs[:, 2] ** 2))
        with np.errstate(divide="ignore", invalid="ignore"):
            cp = np.where(st > 0, vs[:, 0] / st, 1.0); sp = np.where(st > 0, vs[:, 1] / st, 0.0)
        sx, sy = slopes11(self.kind, vs[:, 2], u1, u2)
        rx = (cp * sx - sp * sy) * a; ry = (sp * sx + cp * sy) * a
        m = np.stack([-rx, -ry, np.ones_like(rx)], 1)
        return m / np.linalg.norm(m, axis=1, keepdims=True)


def slopes11(kind, ci, u1, u2):
    """slopes of the alpha = 1 visible normals at cos theta = ci (Heitz, d'Eon 2014): GGX x in closed form and y by inverting its exact conditional
    CDF, Beckmann by inverting the x-slope
    CDF C(x) = ci sqrt(pi)/2 erfc(-x) + si/2 exp(-x^2) on x < cot theta (bisection in float64) and a unit Gaussian / sqrt(2) in y"""
    ci = np.asarray(ci, np.float64); si = np.sqrt(np.maximum(0.0, 1 - ci * ci))
    if kind == GGX:
        with np.errstate(divide="ignore", invalid="ignore"):
            tan = si / ci
            G1 = 2 / (1 + np.sqrt(1 + tan * tan))
            A = 2 * u1 / G1 - 1                                     # in [-1, 1 / cos theta)
            den = A * A - 1
            tmp = 1 / np.where(np.abs(den) < 1e-12, np.copysign(1e-12, den), den)
            D = np.sqrt(np.maximum(tan * tan * tmp * tmp - (A * A - tan * tan) * tmp, 0))
            x1 = tan * tmp - D; x2 = tan * tmp + D
            sx = np.where((A < 0) | (x2 > 1 / tan), x1, x2)
            r = np.sqrt(u1 / (1 - u1)); phi = 2 * np.pi * u2
        normal = ci > 0.9999
        # y given x: sqrt(1 + x^2) tan(phi), phi with density cos^2(phi) / (pi / 2) on (-pi/2, pi/2): phi + sin(phi) cos(phi) = pi (u2 - 1/2)
        lo = np.full_like(u2, -np.pi / 2); hi = np.full_like(u2, np.pi / 2); t = np.pi * (u2 - 0.5)
        for _ in range(80):
            mid = 0.5 * (lo + hi)
            up = mid + np.sin(mid) * np.cos(mid) > t
            hi = np.where(up, mid, hi); lo = np.where(up, lo, mid)
        sy = np.tan(0.5 * (lo + hi)) * np.sqrt(1 + sx * sx)
        return np.where(normal, r * np.cos(phi), sx), np.where(normal, r * np.sin(phi), sy)
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = np.where(si > 0, np.minimum(ci / si, 12.0), 12.0)
    k = 0.5 * np.sqrt(np.pi) * ci
    C = lambda x: k * special.erfc(-x) + 0.5 * si * np.exp(-x * x)
    target = u1 * C(hi)
    lo = np.full_like(hi, -12.0)
    for _ in range(80):
        mid = 0.5 * (lo + hi)
        up = C(mid) > target
        hi = np.where(up, mid, hi); lo = np.where(up, lo, mid)
    return 0.5 * (lo + hi), special.erfinv(np.clip(2 * u2 - 1, -1 + 1e-15, 1 - 1e-15))


def fresnel(cosi, eta):
    """fresnelDielectricExt: (F, cos theta_t) with the sign convention of the reference"""
    cosi = np.asarray(cosi, np.float64)
    scale = np.where(cosi > 0, 1 / eta, eta)
    ct2 = 1 - (1 - cosi * cosi) * scale * scale
    tir = ct2 <= 0
    ci = np.abs(cosi); ct = np.sqrt(np.maximum(ct2, 0))
    with np.errstate(divide="ignore", invalid="ignore"):
        Rs = (ci - eta * ct) / (ci + eta * ct); Rp = (eta * ci - ct) / (eta * ci + ct)
    F = np.where(tir, 1.0, 0.5 * (Rs * Rs + Rp * Rp))
    return F, np.where(tir, 0.0, np.where(cosi > 0, -ct, ct))


def _sampling(d, ci):
    return d if d.visible else d.scaled(1.2 - 0.2 * np.sqrt(np.abs(ci)))


def half_vector(eta, wi, wo):
    """the generalized half vector of (wi, wo) in the upper hemisphere (reflection: wi + wo; refraction: wi + eta' wo)"""
    wi = np.asarray(wi, np.float64); wo = np.asarray(wo, np.float64); eta = np.broadcast_to(np.asarray(eta, np.float64), wi[:, 0].shape)
    refl = wi[:, 2] * wo[:, 2] > 0
    etaR = np.where(refl, 1.0, np.where(wi[:, 2] > 0, eta, 1 / eta))
    H = np.where(refl[:, None], wi + wo, wi + wo * etaR[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        H = H / np.linalg.norm(H, axis=1, keepdims=True)
    return np.where(H[:, 2:3] < 0, -H, H)


def eval_pdf(d, eta, wi, wo):
    """(f |cos theta_o| in ERadiance, solid-angle pdf of the sampler) for arrays wi, wo; eta scalar or per item"""
    wi = np.asarray(wi, np.float64); wo = np.asarray(wo, np.float64); eta = np.broadcast_to(np.asarray(eta, np.float64), wi[:, 0].shape)
    ci, co = wi[:, 2], wo[:, 2]
    refl = ci * co > 0
    etaR = np.where(refl, 1.0, np.where(ci > 0, eta, 1 / eta))
    H = np.where(refl[:, None], wi + wo, wi + wo * etaR[:, None])
    with np.errstate(divide="ignore", invalid="ignore"):
        H = H / np.linalg.norm(H, axis=1, keepdims=True)
    H = np.where(H[:, 2:3] < 0, -H, H)
    D = d.D(H)
    wiH, woH = np.sum(wi * H, 1), np.sum(wo * H, 1)
    F, _ = fresnel(wiH, eta)
    G = d.G1(wi, H) * d.G1(wo, H)
    prob = _sampling(d, ci).pdf_m(np.where(ci[:, None] > 0, wi, -wi), H)
    with np.errstate(divide="ignore", invalid="ignore"):
        sd = wiH + etaR * woH
        factor = np.where(ci > 0, 1 / eta, eta)
        vr = F * D * G / (4 * np.abs(ci))
        vt = np.abs((1 - F) * D * G * etaR ** 2 * wiH * woH / (ci * sd * sd)) * factor ** 2
        pr = np.abs(prob * F / (4 * woH))
        pt = np.abs(prob * (1 - F) * etaR ** 2 * woH / (sd * sd))
    val = np.where(refl, vr, vt); pdf = np.where(refl, pr, pt)
    ok = (ci != 0) & (D > 0) & np.isfinite(val) & np.isfinite(pdf)
    return np.where(ok, val, 0.0), np.where(ok, pdf, 0.0)


def sample(d, eta, wi, u3):
    """(wo, weight = eval / pdf, pdf, eta of the event); u3 = (n, 3): microfacet 2D, reflect / refract choice"""
    wi = np.asarray(wi, np.float64); u3 = np.asarray(u3, np.float64); eta = np.broadcast_to(np.asarray(eta, np.float64), wi[:, 0].shape)
    ci = wi[:, 2]
    sd = _sampling(d, ci)
    ws = np.where(ci[:, None] > 0, wi, -wi)
    if sd.visible:
        m = sd.sample_visible(ws, u3[:, 0], u3[:, 1]); mpdf = sd.pdf_m(ws, m)
    else:
        m = sd.sample_all(u3[:, 0], u3[:, 1]); mpdf = sd.pdf_m(ws, m)
    wiM = np.sum(wi * m, 1)
    F, cosT = fresnel(wiM, eta)
    refl = u3[:, 2] <= F
    e = np.where(cosT < 0, 1 / eta, eta)
    wo_r = m * (2 * wiM)[:, None] - wi
    wo_t = m * (wiM * e + cosT)[:, None] - wi * e[:, None]
    wo = np.where(refl[:, None], wo_r, wo_t)
    etaS = np.where(refl, 1.0, np.where(cosT < 0, eta, 1 / eta))
    woM = np.sum(wo * m, 1)
    with np.errstate(divide="ignore", invalid="ignore"):
        sden = wiM + etaS * woM
        jac = np.where(refl, 1 / (4 * woM), etaS ** 2 * woM / (sden * sden))
        w = np.where(refl, 1.0, np.where(cosT < 0, 1 / eta, eta) ** 2)
        w = w * (d.G1(wo, m) if sd.visible else np.abs(d.D(m) * d.G1(wi, m) * d.G1(wo, m) * wiM / (mpdf * ci)))
    pdf = mpdf * np.where(refl, F, 1 - F) * np.abs(jac)
    bad = (ci == 0) | ~(mpdf > 0) | np.where(refl, ci * wo[:, 2] <= 0, (cosT == 0) | (ci * wo[:, 2] >= 0))
    return wo, np.where(bad, 0.0, w), np.where(bad, 0.0, pdf), etaS


def chi2_pdf(d, eta, wi):
    """pdf_fn of chi2_sphere for one incident direction: the pdf where eval is non-zero (the reference's BSDFAdapter::pdf,
    src/tests/test_chisquare.cpp:212-230 -- pdf() alone is non-zero for some refraction half vectors no sample can produce)"""
    def f(dirs):
        val, pdf = eval_pdf(d, eta, np.repeat(np.asarray(wi, np.float64)[None], len(dirs), 0), dirs)
        return np.where(val > 0, pdf, 0.0)
    return f


def sphere_grid(nt, npp):
    """midpoint grid over the sphere: directions (nt*npp, 3) and their solid angles"""
    th = (np.arange(nt) + 0.5) * np.pi / nt; ph = (np.arange(npp) + 0.5) * 2 * np.pi / npp
    T, Ph = np.meshgrid(th, ph, indexing="ij")
    dirs = np.stack([np.sin(T) * np.cos(Ph), np.sin(T) * np.sin(Ph), np.cos(T)], -1).reshape(-1, 3)
    return dirs, (np.sin(T) * (np.pi / nt) * (2 * np.pi / npp)).reshape(-1)


def albedo(d, eta, wi, nt=1600, npp=800):
    """directional albedo: the integral over the sphere of eval(wi, .) by the midpoint rule"""
    dirs, dw = sphere_grid(nt, npp)
    val, _ = eval_pdf(d, eta, np.repeat(np.asarray(wi, np.float64)[None], len(dirs), 0), dirs)
    return float(np.sum(val * dw))


def chi2_sphere(wo, valid, n, pdf_fn, tb=10, pb=20, m=24):
    """the protocol of the reference's src/tests/test_chisquare.cpp (as tests/test_oracle_kat.py's phase test): a (theta, phi) histogram of
    the valid samples against n x the cell integrals of pdf_fn (midpoint rule, m x m points per cell), cells with an expectation below 5
    pooled.  Returns (p-value, significance level: 1 - (1 - 0.0025)^(1/20), the reference's per-direction level)."""
    wo = np.asarray(wo, np.float64)[valid]
    theta = np.arccos(np.clip(wo[:, 2], -1, 1)); phi = np.arctan2(wo[:, 1], wo[:, 0]); phi[phi < 0] += 2 * np.pi
    ti = np.clip(np.floor(theta * tb / np.pi).astype(int), 0, tb - 1)
    pi_ = np.clip(np.floor(phi * pb / (2 * np.pi)).astype(int), 0, pb - 1)
    table = np.bincount(ti * pb + pi_, minlength=tb * pb).astype(np.float64)
    dirs, dw = sphere_grid(tb * m, pb * m)
    ref = (pdf_fn(dirs) * dw).reshape(tb, m, pb, m).sum((1, 3)).ravel() * n
    chsq, df, pc, pr = 0.0, 0, 0.0, 0.0
    for i in np.argsort(ref):
        e, o = ref[i], table[i]
        if e == 0:
            assert o <= n * 1e-4, (o, n)
        elif e < 5 or (0 < pr < 5):
            pc += o; pr += e
        else:
            chsq += (o - e) ** 2 / e; df += 1
    if pr > 0:
        chsq += (pc - pr) ** 2 / pr; df += 1
    df -= 1
    return 1 - stats.chi2.cdf(chsq, df), 1 - (1 - 0.0025) ** (1.0 / 20)
