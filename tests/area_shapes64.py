"""The three shapes that can carry an `area` emitter -- `rectangle`, `disk`, `sphere` -- restated in numpy from the reference:
rayIntersect (src/shapes/rectangle.cpp:125-148, disk.cpp:139-162, sphere.cpp:163-187), sampleDirect / pdfDirect (src/librender/shape.cpp:
102-126 for the two planar shapes, sphere.cpp:286-384 with warp.cpp:25-31,54-63 for the sphere), the concentric disk map (warp.cpp:81-102)
and the one-sided emitter around them (src/emitters/area.cpp:104-109,158-183).  Written from those lines, not from the HIP code.

Everything is vectorised over N points and evaluated in the dtype `f`: float64 is the yardstick; float32 is the same formulas at the
precision the GPU works in, which the GPU test uses to size its tolerance.  The sphere's ray intersection is solved in double in either
case, as the reference does."""
import numpy as np

EPSILON = 1e-4            # Epsilon of a single-precision build (include/mitsuba/core/constants.h)
RECT, DISK, SPHERE = "rectangle", "disk", "sphere"


def _dot(a, b):
    return (a * b).sum(axis=-1)


def _norm(a):
    return np.sqrt(_dot(a, a))


class Shape:
    """kind, the 3x4 / 4x4 toWorld and the radiance.  A sphere has its centre at the translation column and the radius |toWorld e_x|
    (sphere.cpp:113-122); a linear part of negative determinant flips the normals (disk.cpp:86-87 does flipNormals that way)."""

    def __init__(self, kind, to_world, radiance):
        m = np.eye(4); t = np.asarray(to_world, np.float64); m[:t.shape[0], :4] = t
        m = m.astype(np.float32).astype(np.float64)                       # what the float32 C structs carry
        self.kind, self.M, self.L = kind, m[:3, :4], np.asarray(radiance, np.float64)
        A = m[:3, :3]
        self.W = np.linalg.inv(m)[:3, :4]
        n = np.linalg.inv(A).T @ np.array([0.0, 0.0, 1.0])                # toWorld(Normal(0,0,1)): the inverse transpose
        self.n = n / np.linalg.norm(n)
        lu, lv = np.linalg.norm(A[:, 0]), np.linalg.norm(A[:, 1])
        self.c = m[:3, 3].copy()
        self.R = float(np.float32(lu))
        self.flip = -1.0 if np.linalg.det(A) < 0 else 1.0
        self.inv_area = {RECT: 1.0 / (4 * lu * lv), DISK: 1.0 / (np.pi * lu * lu), SPHERE: 1.0 / (4 * np.pi * lu * lu)}[kind]


def sphere(center, radius, radiance, flip=False):
    m = np.eye(4); m[0, 0] = m[1, 1] = radius; m[2, 2] = -radius if flip else radius; m[:3, 3] = center
    return Shape(SPHERE, m, radiance)


def concentric(u, f=np.float64):
    """warp::squareToUniformDiskConcentric"""
    u = np.asarray(u, f)
    r1, r2 = f(2) * u[:, 0] - f(1), f(2) * u[:, 1] - f(1)
    first = r1 * r1 > r2 * r2
    with np.errstate(divide="ignore", invalid="ignore"):
        phi = np.where(first, f(np.pi / 4) * (r2 / r1), f(np.pi / 2) - (r1 / r2) * f(np.pi / 4))
    r = np.where(first, r1, r2)
    zero = (r1 == 0) & (r2 == 0)
    phi = np.where(zero, f(0), phi).astype(f); r = np.where(zero, f(0), r).astype(f)
    return r * np.cos(phi), r * np.sin(phi)


def uniform_sphere(u, f=np.float64):
    """warp::squareToUniformSphere"""
    u = np.asarray(u, f)
    z = f(1) - f(2) * u[:, 1]
    r = np.sqrt(np.maximum(f(1) - z * z, f(0)))
    phi = f(2 * np.pi) * u[:, 0]
    return np.stack([r * np.cos(phi), r * np.sin(phi), z], axis=1).astype(f)


def frame(a, f=np.float64):
    """coordinateSystem (src/libcore/util.cpp:606-615): s, t with (s, t, a) right-handed"""
    x, y, z = a[:, 0], a[:, 1], a[:, 2]
    big = np.abs(x) > np.abs(y)
    with np.errstate(divide="ignore", invalid="ignore"):
        il1 = f(1) / np.sqrt(x * x + z * z); il2 = f(1) / np.sqrt(y * y + z * z)
    zero = np.zeros_like(x)
    c = np.where(big[:, None], np.stack([z * il1, zero, -x * il1], 1), np.stack([zero, z * il2, -y * il2], 1)).astype(f)
    b = np.cross(c, a).astype(f)
    return b, c


def intersect(sh, o, d, mint=0.0, maxt=np.inf, f=np.float64):
    """rayIntersect: t in [mint, maxt], or -1"""
    o = np.asarray(o, f); d = np.asarray(d, f)
    maxt = np.broadcast_to(np.asarray(maxt, np.float64), o.shape[:1])
    if sh.kind == SPHERE:                                                  # in double whatever f is (sphere.cpp:164-172)
        oo = o.astype(np.float64) - sh.c.astype(f).astype(np.float64); dd = d.astype(np.float64)
        R = np.float64(f(sh.R))
        A, B, C = _dot(dd, dd), 2 * _dot(oo, dd), _dot(oo, oo) - R * R
        disc = B * B - 4 * A * C
        ok = disc >= 0
        root = np.sqrt(np.where(ok, disc, 0.0))
        temp = np.where(B < 0, -0.5 * (B - root), -0.5 * (B + root))
        with np.errstate(divide="ignore", invalid="ignore"):
            x0, x1 = temp / A, C / temp
        near, far = np.minimum(x0, x1), np.maximum(x0, x1)
        ok = ok & (near <= maxt) & (far >= mint)
        use_far = near < mint
        ok = ok & ~(use_far & (far > maxt))
        return np.where(ok, np.where(use_far, far, near), -1.0).astype(f)
    W = sh.W.astype(f)
    lo = o @ W[:, :3].T + W[:, 3]; ld = d @ W[:, :3].T
    with np.errstate(divide="ignore", invalid="ignore"):
        hit = -lo[:, 2] / ld[:, 2]
    ok = (hit >= mint) & (hit <= maxt)
    lx, ly = lo[:, 0] + hit * ld[:, 0], lo[:, 1] + hit * ld[:, 1]
    inside = (lx * lx + ly * ly <= 1) if sh.kind == DISK else ((np.abs(lx) <= 1) & (np.abs(ly) <= 1))
    return np.where(ok & inside, hit, f(-1)).astype(f)


def normal_at(sh, p, f=np.float64):
    if sh.kind != SPHERE:
        return np.broadcast_to(sh.n.astype(f), p.shape).copy()
    v = np.asarray(p, f) - sh.c.astype(f)
    return (v / _norm(v)[:, None] * f(sh.flip)).astype(f)


def radiance(sh, p, d, f=np.float64):
    """AreaLight::eval: the radiance a ray travelling along d picks up at the surface point p (one-sided)"""
    front = _dot(normal_at(sh, p, f), -np.asarray(d, f)) > 0
    return np.where(front[:, None], sh.L.astype(f), f(0)).astype(f)


def sample_direct(sh, ref, u, f=np.float64):
    """AreaLight::sampleDirect for refN = 0: radiance / pdf (0 from the back), d, dist, the solid-angle pdf (0 from the back), n"""
    ref = np.asarray(ref, f); u = np.asarray(u, f)
    if sh.kind == SPHERE:
        c, R = sh.c.astype(f), f(sh.R)
        r2c = c - ref
        refDist2 = _dot(r2c, r2c); invRefDist = f(1) / np.sqrt(refDist2)
        sinAlpha = R * invRefDist
        outside = sinAlpha < f(1 - EPSILON)
        # the cone of directions that contains the sphere (sphere.cpp:295-334)
        cosAlpha = np.sqrt(np.maximum(f(1) - sinAlpha * sinAlpha, f(0)))
        cosTheta = (f(1) - u[:, 0]) + u[:, 0] * cosAlpha
        sinTheta = np.sqrt(np.maximum(f(1) - cosTheta * cosTheta, f(0)))
        phi = f(2 * np.pi) * u[:, 1]
        a = r2c * invRefDist[:, None]
        s, t = frame(a, f)
        d1 = s * (np.cos(phi) * sinTheta)[:, None] + t * (np.sin(phi) * sinTheta)[:, None] + a * cosTheta[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf1 = f(1 / (2 * np.pi)) / (f(1) - cosAlpha)
            baseT = refDist2 / _dot(r2c, d1)
        q2c = c - (ref + d1 * baseT[:, None])
        qProj = _dot(q2c, d1)
        B, C = f(-2) * qProj, _dot(q2c, q2c) - R * R
        disc = B * B - f(4) * C
        root = np.sqrt(np.maximum(disc, f(0)))
        temp = np.where(B < 0, f(-0.5) * (B - root), f(-0.5) * (B + root))
        with np.errstate(divide="ignore", invalid="ignore"):
            nearT = np.where(disc >= 0, np.fmin(temp, C / temp), qProj)
        dist1 = baseT + nearT
        n1 = d1 * nearT[:, None] - q2c
        with np.errstate(divide="ignore", invalid="ignore"):
            n1 = n1 / _norm(n1)[:, None]
        # uniformly by area (sphere.cpp:335-349)
        n2 = uniform_sphere(u, f)
        d2 = c + n2 * R - ref
        dist2sq = _dot(d2, d2); dist2 = np.sqrt(dist2sq)
        d2 = d2 / dist2[:, None]
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf2 = f(sh.inv_area) * dist2sq / np.abs(_dot(d2, n2))
        o = outside[:, None]
        d, n = np.where(o, d1, d2).astype(f), (np.where(o, n1, n2) * f(sh.flip)).astype(f)
        dist, pdf = np.where(outside, dist1, dist2).astype(f), np.where(outside, pdf1, pdf2).astype(f)
    else:
        if sh.kind == DISK:
            lx, ly = concentric(u, f)
        else:
            lx, ly = u[:, 0] * f(2) - f(1), u[:, 1] * f(2) - f(1)
        M = sh.M.astype(f)
        p = lx[:, None] * M[:, 0] + ly[:, None] * M[:, 1] + M[:, 3]
        n = np.broadcast_to(sh.n.astype(f), p.shape).copy()
        d = p - ref
        distSq = _dot(d, d); dist = np.sqrt(distSq)
        d = d / dist[:, None]
        dp = np.abs(_dot(d, n))
        with np.errstate(divide="ignore", invalid="ignore"):
            pdf = f(sh.inv_area) * np.where(dp != 0, distSq / dp, f(0))
    ok = (_dot(d, n) < 0) & (pdf != 0)
    with np.errstate(divide="ignore", invalid="ignore"):
        value = np.where(ok[:, None], sh.L.astype(f) / pdf[:, None], f(0)).astype(f)
    return value, d.astype(f), dist.astype(f), np.where(ok, pdf, f(0)).astype(f), n.astype(f)


def pdf_direct(sh, ref, d, dist, f=np.float64):
    """AreaLight::pdfDirect in the solid-angle measure of the surface point ref + dist d seen from ref"""
    ref = np.asarray(ref, f); d = np.asarray(d, f); dist = np.asarray(dist, f)
    n = normal_at(sh, ref + d * dist[:, None], f)
    dn = _dot(d, n)
    with np.errstate(divide="ignore", invalid="ignore"):
        pdf = f(sh.inv_area) * dist * dist / np.abs(dn)
        if sh.kind == SPHERE:
            r2c = sh.c.astype(f) - ref
            sinAlpha = f(sh.R) * (f(1) / _norm(r2c))
            cosAlpha = np.sqrt(np.maximum(f(1) - sinAlpha * sinAlpha, f(0)))
            pdf = np.where(sinAlpha < f(1 - EPSILON), f(1 / (2 * np.pi)) / (f(1) - cosAlpha), pdf)
    return np.where(dn < 0, pdf, f(0)).astype(f)


def nearest(shapes, o, d, mint=0.0, maxt=np.inf, f=np.float64):
    """the nearest of the shapes along o + t d: (index or -1, t or -1); ties go to the first listed"""
    o = np.asarray(o, f)
    best = np.full(o.shape[0], -1.0, f); idx = np.full(o.shape[0], -1)
    for j, sh in enumerate(shapes):
        t = intersect(sh, o, d, mint, maxt, f)
        take = (t >= 0) & ((best < 0) | (t < best))
        best = np.where(take, t, best).astype(f); idx = np.where(take, j, idx)
    return idx, best
