"""The exitance map of mer_render_exitance restated in float64 with numpy, for a grey homogeneous medium with the null boundary in the cube
[-1, 1]^3 or in a sphere about the origin (include/mer.h, mer_render_exitance, has the estimator).  Vectorised over the paths of a batch;
independent of the library.

The walk is tests/fluence64.py's (render): emission, one depth and one roulette trip for the null boundary when the emitter lies outside,
free flights t ~ sigma_t exp(-sigma_t t) (sigma_t = 0: every flight reaches the boundary), albedo, Henyey-Greenstein, roulette.  What is
new is what happens when a flight passes the exit of the shape: the exit point x, the direction d, the weight w = T power and the optical
path length l (exterior leg at index 1, every flight inside times the constant index n) go through the cone (c = d . normal < cos_min:
`rejected`), the window (frame = floor((l - t_min) / t_bin) outside 0 ... frames - 1: `late`) and into the cell of x.  An emitted ray that
misses the shape adds its weight to `missed` (and, as in the fluence grids, to `escaped`).

Totals (16, as mer_exitance_read): [0] paths, [1..3] escaped, [4..6] missed, [7] ended (always 0 here), [8..10] late, [11..13] rejected,
[14] exits binned, [15] 0."""
import numpy as np
from tests.fluence64 import point, collimated, hg_sample, bar, total_bar       # noqa: F401  (re-exported for the tests)

CUBE = ("cube",)


def sphere(radius):
    return ("sphere", float(radius))


def faces(shape):
    return 6 if shape[0] == "cube" else 1


def _span(x, d, shape):
    """entry and exit parameters of the rays x + t d against the shape, and whether the line meets it"""
    if shape[0] == "cube":
        with np.errstate(divide="ignore", invalid="ignore"):
            inv = 1.0 / np.where(d == 0, 1e-300, d)
        a, b = (-1.0 - x) * inv, (1.0 - x) * inv
        tn, tf = np.minimum(a, b).max(1), np.maximum(a, b).min(1)
        return tn, tf, tn <= tf
    R = shape[1]
    b = (x * d).sum(1); c = (x * x).sum(1) - R * R
    disc = b * b - c
    root = np.sqrt(np.maximum(disc, 0))
    return -b - root, -b + root, disc > 0


def _inside(x, shape):
    return np.all(np.abs(x) <= 1) if shape[0] == "cube" else (x * x).sum() < shape[1] ** 2


def normal(x, shape):
    """outward normal at the surface points x: cube, the axis on which |x| is largest (first on a tie), sign + when x >= 0"""
    if shape[0] == "sphere":
        return x / np.linalg.norm(x, axis=1, keepdims=True)
    axis = np.argmax(np.abs(x), 1)
    n = np.zeros_like(x)
    n[np.arange(len(x)), axis] = np.where(x[np.arange(len(x)), axis] >= 0, 1.0, -1.0)
    return n


def cell(x, shape, res):
    """flat index (face, iv, iu) of the surface points x; res = (res_u, res_v)"""
    ru, rv = res
    if shape[0] == "sphere":
        q = x / np.linalg.norm(x, axis=1, keepdims=True)
        a = np.arctan2(q[:, 1], q[:, 0]) / (2 * np.pi)
        a = np.where(a < 0, a + 1, a)
        iu = np.clip(np.floor(a * ru), 0, ru - 1).astype(np.int64)
        iv = np.clip(np.floor(0.5 * (1 + q[:, 2]) * rv), 0, rv - 1).astype(np.int64)
        return iv * ru + iu
    rows = np.arange(len(x))
    axis = np.argmax(np.abs(x), 1)
    face = 2 * axis + (x[rows, axis] >= 0)
    xu, xv = x[rows, (axis + 1) % 3], x[rows, (axis + 2) % 3]
    iu = np.clip(np.floor((xu + 1) / 2 * ru), 0, ru - 1).astype(np.int64)
    iv = np.clip(np.floor((xv + 1) / 2 * rv), 0, rv - 1).astype(np.int64)
    return (face * rv + iv) * ru + iu


def render(emitter, sigma_s, sigma_a, g, shape, res, frames=1, t_min=0.0, t_bin=0.0, cos_min=0.0, n=1.0, paths=4096, batches=16, seed=0,
           max_depth=-1, rr_depth=5, max_events=4096, counts=False):
    """`batches` independent batches of `paths` paths: (sums (batches, frames, faces, res_v, res_u), totals (batches, 16)): raw sums as the
    library keeps them (one channel: the medium is grey; the three channels of the totals are equal).  counts = True: a third array shaped
    like sums, the number of exits binned per key"""
    rng = np.random.default_rng(seed)
    st = float(sigma_s + sigma_a); albedo = float(sigma_s) / st if st > 0 else 0.0
    nf = faces(shape); ncell = nf * res[0] * res[1]
    sums = np.zeros((batches, frames * ncell)); hits = np.zeros((batches, frames * ncell)); totals = np.zeros((batches, 16))
    outside = not _inside(emitter["o"], shape)
    phi = emitter["phi"]
    for b in range(batches):
        N = paths
        totals[b, 0] = N
        if emitter["kind"] == "point":
            w = rng.random((N, 2)); z = 1 - 2 * w[:, 0]; ph = 2 * np.pi * w[:, 1]; rr = np.sqrt(np.maximum(1 - z * z, 0))
            d = np.stack([rr * np.cos(ph), rr * np.sin(ph), z], 1)
        else:
            d = np.tile(emitter["d"], (N, 1))
        x = np.tile(emitter["o"], (N, 1))
        T = np.ones(N); L = np.zeros(N)
        depth = 1
        if outside:                                                     # to the null boundary: one depth, one roulette trip
            tn, tf, meets = _span(x, d, shape)
            hit = meets & (tn > 0)
            totals[b, 4:7] += phi * np.count_nonzero(~hit); totals[b, 1:4] += phi * np.count_nonzero(~hit)
            x, d, T, L = x[hit] + d[hit] * tn[hit, None], d[hit], T[hit], tn[hit]
            if depth >= rr_depth:
                q = np.minimum(T, 0.95); keep = rng.random(len(T)) < q
                x, d, T, L = x[keep], d[keep], T[keep] / q[keep], L[keep]
            depth += 1
        for _ in range(max_events):
            if len(T) == 0 or not (depth <= max_depth or max_depth < 0):
                break
            _, tex, _m = _span(x, d, shape)
            u = rng.random(len(T))
            tfl = -np.log1p(-u) / st if st > 0 else np.full(len(T), np.inf)
            sc = tfl < tex
            # ---- the exits
            ex = ~sc
            xe = x[ex] + d[ex] * tex[ex, None]; de = d[ex]; we = phi * T[ex]; le = L[ex] + tex[ex] * n
            totals[b, 1:4] += we.sum()
            c = (de * normal(xe, shape)).sum(1)
            rej = (c < cos_min) if cos_min > 0 else np.zeros(len(we), bool)
            totals[b, 11:14] += we[rej].sum()
            if t_bin > 0:
                fr = np.floor((le - t_min) / t_bin)
                late = ~rej & ~((fr >= 0) & (fr < frames))
            else:
                fr = np.zeros(len(we)); late = np.zeros(len(we), bool)
            totals[b, 8:11] += we[late].sum()
            ok = ~rej & ~late
            key = fr[ok].astype(np.int64) * ncell + cell(xe[ok], shape, res)
            sums[b] += np.bincount(key, we[ok], frames * ncell)
            hits[b] += np.bincount(key, None, frames * ncell)
            totals[b, 14] += np.count_nonzero(ok)
            # ---- the collisions
            x, d, T, L = x[sc] + d[sc] * tfl[sc, None], d[sc], T[sc] * albedo, L[sc] + tfl[sc] * n
            live = T > 0
            x, d, T, L = x[live], d[live], T[live], L[live]
            if len(T) == 0:
                break
            d = hg_sample(g, d, rng.random((len(T), 2)))
            if depth >= rr_depth:
                q = np.minimum(T, 0.95); keep = rng.random(len(T)) < q
                x, d, T, L = x[keep], d[keep], T[keep] / q[keep], L[keep]
            depth += 1
    shp = (batches, frames, nf, res[1], res[0])
    return (sums.reshape(shp), totals, hits.reshape(shp)) if counts else (sums.reshape(shp), totals)


def identity_gap(sums, totals):
    """per batch: sum(sums) + missed + rejected + late - escaped, relative to escaped"""
    lhs = sums.reshape(len(sums), -1).sum(1) + totals[:, 4] + totals[:, 11] + totals[:, 8]
    return np.abs(lhs - totals[:, 1]) / np.maximum(totals[:, 1], 1e-300)


def cube_cell_solid_angles(res):
    """solid angle of every cell of one face of the cube [-1, 1]^3 seen from the centre, (res_v, res_u): with the face at distance 1 and the
    cell [u0, u1] x [v0, v1], Omega = sum over the corners of +- atan(u v / sqrt(1 + u^2 + v^2)); the face's cells sum to 4 pi / 6"""
    ru, rv = res
    u = -1 + 2 * np.arange(ru + 1) / ru; v = -1 + 2 * np.arange(rv + 1) / rv
    U, V = np.meshgrid(u, v)                                              # (rv + 1, ru + 1)
    A = np.arctan(U * V / np.sqrt(1 + U * U + V * V))
    return A[1:, 1:] - A[1:, :-1] - A[:-1, 1:] + A[:-1, :-1]


def cell_rect(face, iv, iu, res):
    """the rectangle of a cube cell as (lo, hi) corners in 3-D"""
    axis = face // 2; ua, va = (axis + 1) % 3, (axis + 2) % 3
    lo = np.zeros(3); hi = np.zeros(3)
    lo[axis] = hi[axis] = 1.0 if face % 2 else -1.0
    lo[ua], hi[ua] = -1 + 2 * iu / res[0], -1 + 2 * (iu + 1) / res[0]
    lo[va], hi[va] = -1 + 2 * iv / res[1], -1 + 2 * (iv + 1) / res[1]
    return lo, hi
