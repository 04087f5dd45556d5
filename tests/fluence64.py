"""The fluence grid of mer_render_fluence restated in float64 with numpy, for a grey homogeneous medium in the cube [-1, 1]^3 with the null
boundary (include/mer.h, mer_render_fluence, has the estimator).  Vectorised over the paths of a batch; independent of the library.

A path: emitted by a collimated beam (the fixed ray, weight = power) or a point emitter (uniform sphere, weight = 4 pi I); an emitter
outside the cube pays one depth for the null boundary (and a roulette trip); then, while depth <= max_depth (or max_depth < 0): a free
flight t ~ sigma_t exp(-sigma_t t) (medium_sampling_weight = 1), escape if it passes the exit, else a real collision: the deposit
w = T power / sigma_t into the cell that holds the point (half-open cells, floor((p - bmin) / (bmax - bmin) res); outside the box: into
`dropped`), T *= albedo, a Henyey-Greenstein direction, and the roulette: from depth >= rr_depth on the path survives with q = min(T, 0.95)
and T /= q.  T is the throughput WITHOUT the power, as the light tracer's roulette has it.

Totals (8, as mer_fluence_read): paths started, escaped weight x 3, dropped deposit weight x 3, paths ended by a budget (always 0 here)."""
import numpy as np


def point(position, intensity):
    return {"kind": "point", "o": np.asarray(position, np.float64), "phi": 4.0 * np.pi * float(intensity)}


def collimated(origin, direction, power):
    d = np.asarray(direction, np.float64)
    return {"kind": "collimated", "o": np.asarray(origin, np.float64), "d": d / np.linalg.norm(d), "phi": float(power)}


def _slabs(x, d):
    """entry and exit parameters of the rays x + t d against the cube (float64; a zero component never divides)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / np.where(d == 0, 1e-300, d)
    a, b = (-1.0 - x) * inv, (1.0 - x) * inv
    return np.minimum(a, b).max(1), np.maximum(a, b).min(1)


def hg_sample(g, d, u):
    """a direction whose cosine mu to d has the density (1 - g^2) / (2 (1 + g^2 - 2 g mu)^1.5) (g = 0: uniform)"""
    if g == 0:
        mu = 1 - 2 * u[:, 0]
    else:
        s = (1 - g * g) / (1 - g + 2 * g * u[:, 0])
        mu = (1 + g * g - s * s) / (2 * g)
    a = np.where(np.abs(d[:, :1]) < 0.9, np.array([[1.0, 0.0, 0.0]]), np.array([[0.0, 1.0, 0.0]]))
    s1 = np.cross(a, d); s1 /= np.linalg.norm(s1, axis=1, keepdims=True); t1 = np.cross(d, s1)
    sn = np.sqrt(np.maximum(1 - mu * mu, 0)); ph = 2 * np.pi * u[:, 1]
    return s1 * (sn * np.cos(ph))[:, None] + t1 * (sn * np.sin(ph))[:, None] + d * mu[:, None]


def cells(p, res, bmin, bmax):
    """(flat index [z][y][x], inside) of the points p: half-open cells"""
    res = np.asarray(res); bmin = np.asarray(bmin, np.float64); bmax = np.asarray(bmax, np.float64)
    i = np.floor((p - bmin) / (bmax - bmin) * res).astype(np.int64)
    inside = np.all((i >= 0) & (i < res), axis=1)
    i = np.where(inside[:, None], i, 0)
    return (i[:, 2] * res[1] + i[:, 1]) * res[0] + i[:, 0], inside


def render(emitter, sigma_s, sigma_a, g, res, bmin=(-1, -1, -1), bmax=(1, 1, 1), paths=4096, batches=16, seed=0, max_depth=-1, rr_depth=5,
           max_events=4096):
    """`batches` independent batches of `paths` paths: (sums (batches, nz, ny, nx), totals (batches, 8)), raw sums as the library keeps
    them (one channel: the medium is grey; the three channels of the totals are equal)"""
    rng = np.random.default_rng(seed)
    st = float(sigma_s + sigma_a); albedo = float(sigma_s) / st
    ncell = int(np.prod(res))
    sums = np.zeros((batches, ncell)); totals = np.zeros((batches, 8))
    outside = not np.all(np.abs(emitter["o"]) <= 1)
    for b in range(batches):
        N = paths
        totals[b, 0] = N
        if emitter["kind"] == "point":
            w = rng.random((N, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(np.maximum(1 - z * z, 0))
            d = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
        else:
            d = np.tile(emitter["d"], (N, 1))
        x = np.tile(emitter["o"], (N, 1))
        T = np.ones(N); phi = emitter["phi"]
        depth = 1
        escaped = 0.0; dropped = 0.0
        if outside:                                                     # to the null boundary: one depth, one roulette trip
            tn, tf = _slabs(x, d)
            hit = (tn <= tf) & (tn > 0)
            escaped += phi * np.count_nonzero(~hit)
            x, d, T = x[hit] + d[hit] * tn[hit, None], d[hit], T[hit]
            if depth >= rr_depth:
                q = np.minimum(T, 0.95); keep = rng.random(len(T)) < q
                x, d, T = x[keep], d[keep], T[keep] / q[keep]
            depth += 1
        for _ in range(max_events):
            if len(T) == 0 or not (depth <= max_depth or max_depth < 0):
                break
            _, tex = _slabs(x, d)
            tfl = -np.log1p(-rng.random(len(T))) / st
            sc = tfl < tex
            escaped += phi * T[~sc].sum()
            x, d, T = x[sc] + d[sc] * tfl[sc, None], d[sc], T[sc]
            if len(T) == 0:
                break
            idx, inside = cells(x, res, bmin, bmax)
            wdep = T * phi / st
            sums[b] += np.bincount(idx[inside], wdep[inside], ncell)
            dropped += wdep[~inside].sum()
            T = T * albedo
            live = T > 0
            x, d, T = x[live], d[live], T[live]
            d = hg_sample(g, d, rng.random((len(T), 2)))
            if depth >= rr_depth:
                q = np.minimum(T, 0.95); keep = rng.random(len(T)) < q
                x, d, T = x[keep], d[keep], T[keep] / q[keep]
            depth += 1
        totals[b, 1:4] = escaped; totals[b, 4:7] = dropped
    return sums.reshape((batches, res[2], res[1], res[0])), totals


def beam_column(emitter, sigma_t, res, bmin=(-1, -1, -1), bmax=(1, 1, 1)):
    """closed form for a beam along +z: per path, the probability p[z][y][x] that its FIRST collision falls into the cell (Beer-Lambert over the
    cell's z interval clipped to the cube, counted from the entry face z = -1), zero off the beam's column.  A cell's expected sum per path
    is P / sigma_t p, its variance (P / sigma_t)^2 p (1 - p)."""
    assert emitter["kind"] == "collimated" and np.allclose(emitter["d"], [0, 0, 1])
    res = np.asarray(res); bmin = np.asarray(bmin, np.float64); bmax = np.asarray(bmax, np.float64)
    o = emitter["o"]
    p = np.zeros((res[2], res[1], res[0]))
    if not (abs(o[0]) <= 1 and abs(o[1]) <= 1):
        return p
    ij = np.floor((o[:2] - bmin[:2]) / (bmax[:2] - bmin[:2]) * res[:2]).astype(int)
    if np.any(ij < 0) or np.any(ij >= res[:2]):
        return p
    edges = bmin[2] + (bmax[2] - bmin[2]) * np.arange(res[2] + 1) / res[2]
    z0 = max(-1.0, float(o[2]))
    a = np.clip(edges[:-1], z0, 1.0) - z0; b = np.clip(edges[1:], z0, 1.0) - z0
    p[:, ij[1], ij[0]] = np.exp(-sigma_t * a) - np.exp(-sigma_t * b)
    return p


def bar(mean, sd, ref, ref_var=0.0, what=""):
    """the project's bar (tests/test_gpu_ptracer.py, _bar) for `mean` (standard deviation of the mean `sd`) against `ref` (variance ref_var):
    at most 1 + 1 % of the cells beyond 4 sigma, with the floor 1e-7 max|ref| under sigma; returns z"""
    s = np.sqrt(sd * sd + ref_var)
    floor = 1e-7 * max(float(np.abs(ref).max()), 1e-30)
    z = np.abs(mean - ref) / np.maximum(s, floor)
    print("%s: %d of %d beyond 4 sigma, max z %.2f" % (what, (z > 4).sum(), z.size, z.max()))
    assert (z > 4).sum() <= 1 + 0.01 * z.size, (what, np.sort(z.ravel())[-5:])
    return z


def total_bar(totals, ref, ref_var=0.0, what=""):
    """a total over K batches against `ref`: z <= 4 (_total_bar)"""
    zt = abs(totals.mean() - ref) / np.sqrt(totals.var(ddof=1) / len(totals) + ref_var)
    print("%s: total z %.2f (mean / ref = %.5f)" % (what, zt, totals.mean() / ref))
    assert zt <= 4, (what, zt)
    return zt
