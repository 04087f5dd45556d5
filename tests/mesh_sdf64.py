"""float64 reference of mer_sdf_from_mesh (include/mer.h): per grid node the minimum over the triangles of the point-triangle distance
(closest point by Voronoi regions, Ericson, Real-Time Collision Detection 5.1.5) and the generalized winding number
w = (1 / 4 pi) sum_t 2 atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|), a, b, c = the vertices minus the node
(Van Oosterom-Strackee); inside iff |w| >= 0.5; the grid holds -distance inside, +distance outside.

It starts where the library starts: the float32 node coordinates aabb_min + (float) i * ((aabb_max - aabb_min) / (float) (res - 1)) and the
float32 vertices, both upcast to float64.  Everything after that is float64 numpy, one triangle at a time over all nodes.

Also the meshes the tests use, generated here: a 12-triangle cube and an icosphere by subdivision."""
import numpy as np


def node_coords(res, aabb_min, aabb_max):
    """float32 node coordinates per axis, by the library's expression"""
    out = []
    for a in range(3):
        lo, hi = np.float32(aabb_min[a]), np.float32(aabb_max[a])
        step = np.float32(np.float32(hi - lo) / np.float32(res[a] - 1))
        out.append((lo + np.arange(res[a], dtype=np.float32) * step).astype(np.float32))
    return out


def nodes(res, aabb_min, aabb_max):
    """float64 [nz][ny][nx][3] node positions (upcast float32 coordinates)"""
    x, y, z = node_coords(res, aabb_min, aabb_max)
    Z, Y, X = np.meshgrid(z.astype(np.float64), y.astype(np.float64), x.astype(np.float64), indexing="ij")
    return np.stack([X, Y, Z], -1)


def _dot(u, v):
    return (u * v).sum(-1)


def point_triangle_dist2(p, A, B, C):
    """squared distance of the points p [...,3] to the triangle A B C: Ericson 5.1.5, regions tested in the book's order"""
    a, b, c = A - p, B - p, C - p
    ab, ac = b - a, c - a
    d1, d2 = -_dot(ab, a), -_dot(ac, a)
    d3, d4 = -_dot(ab, b), -_dot(ac, b)
    d5, d6 = -_dot(ab, c), -_dot(ac, c)
    vc = d1 * d4 - d3 * d2; vb = d5 * d2 - d1 * d6; va = d3 * d6 - d5 * d4
    one, zero = np.ones_like(d1), np.zeros_like(d1)
    conds = [(d1 <= 0) & (d2 <= 0), (d3 >= 0) & (d4 <= d3), (vc <= 0) & (d1 >= 0) & (d3 <= 0), (d6 >= 0) & (d5 <= d6),
             (vb <= 0) & (d2 >= 0) & (d6 <= 0), (va <= 0) & (d4 - d3 >= 0) & (d5 - d6 >= 0)]
    ns = np.select(conds, [zero, one, d1, zero, zero, d5 - d6], vb)
    nt = np.select(conds, [zero, zero, zero, one, d2, d4 - d3], vc)
    den = np.select(conds, [one, one, d1 - d3, one, d2 - d6, (d4 - d3) + (d5 - d6)], (va + vb) + vc)
    with np.errstate(divide="ignore", invalid="ignore"):
        s, t = ns / den, nt / den
    q = a + ab * s[..., None] + ac * t[..., None]
    return _dot(q, q)


def half_solid_angle(p, A, B, C):
    a, b, c = A - p, B - p, C - p
    la, lb, lc = np.sqrt(_dot(a, a)), np.sqrt(_dot(b, b)), np.sqrt(_dot(c, c))
    num = _dot(a, np.cross(b, c))
    den = la * lb * lc + _dot(a, b) * lc + _dot(b, c) * la + _dot(c, a) * lb
    return np.arctan2(num, den)


def mesh_sdf64(vertices, triangles, res, aabb_min, aabb_max):
    """-> (sdf [nz][ny][nx], w [nz][ny][nx]) in float64"""
    p = nodes(res, aabb_min, aabb_max)
    v = np.asarray(vertices, np.float32).astype(np.float64)
    d2 = np.full(p.shape[:3], np.inf)
    s = np.zeros(p.shape[:3])
    for i0, i1, i2 in np.asarray(triangles).reshape(-1, 3):
        d2 = np.minimum(d2, point_triangle_dist2(p, v[i0], v[i1], v[i2]))
        s = s + 2.0 * half_solid_angle(p, v[i0], v[i1], v[i2])
    w = s / (4.0 * np.pi)
    d = np.sqrt(d2)
    return np.where(np.abs(w) >= 0.5, -d, d), w


# ---- meshes -------------------------------------------------------------------------------------------
def cube(h=1.0):
    """the cube [-h, h]^3 as 12 triangles, outward orientation; the last two triangles are the face z = +h"""
    v = np.array([[x, y, z] for z in (-h, h) for y in (-h, h) for x in (-h, h)], np.float32)      # index = x + 2 y + 4 z
    quads = [(0, 4, 6, 2), (1, 3, 7, 5), (0, 1, 5, 4), (2, 6, 7, 3), (0, 2, 3, 1), (4, 5, 7, 6)]      # -x +x -y +y -z +z
    t = []
    for a, b, c, d in quads:
        t += [[a, b, c], [a, c, d]]
    return v, np.array(t, np.int32)


def _subdivide(v, t, radius):
    v = [tuple(x) for x in v]
    mid = {}

    def m(i, j):
        k = (min(i, j), max(i, j))
        if k not in mid:
            q = (np.array(v[i], np.float64) + np.array(v[j], np.float64)) / 2
            if radius is not None:
                q = q * (radius / np.linalg.norm(q))
            mid[k] = len(v); v.append(tuple(q))
        return mid[k]
    out = []
    for a, b, c in t:
        ab, bc, ca = m(a, b), m(b, c), m(c, a)
        out += [[a, ab, ca], [b, bc, ab], [c, ca, bc], [ab, bc, ca]]
    return np.array(v, np.float64), np.array(out, np.int32)


def icosphere(radius=0.9, subdivisions=2):
    """icosahedron subdivided `subdivisions` times, the new vertices pushed to the sphere: 20 * 4^s triangles, outward orientation"""
    g = (1.0 + 5.0 ** 0.5) / 2.0
    v = np.array([[-1, g, 0], [1, g, 0], [-1, -g, 0], [1, -g, 0], [0, -1, g], [0, 1, g], [0, -1, -g], [0, 1, -g],
                  [g, 0, -1], [g, 0, 1], [-g, 0, -1], [-g, 0, 1]], np.float64)
    v *= radius / np.linalg.norm(v[0])
    t = np.array([[0, 11, 5], [0, 5, 1], [0, 1, 7], [0, 7, 10], [0, 10, 11], [1, 5, 9], [5, 11, 4], [11, 10, 2], [10, 7, 6], [7, 1, 8],
                  [3, 9, 4], [3, 4, 2], [3, 2, 6], [3, 6, 8], [3, 8, 9], [4, 9, 5], [2, 4, 11], [6, 2, 10], [8, 6, 7], [9, 8, 1]], np.int32)
    for _ in range(subdivisions):
        v, t = _subdivide(v, t, radius)
    return v.astype(np.float32), t


def box_sdf(p, h=1.0):
    """closed-form signed distance (negative inside) of the points p [...,3] to the cube [-h, h]^3"""
    q = np.abs(p) - h
    return np.linalg.norm(np.maximum(q, 0.0), axis=-1) + np.minimum(q.max(-1), 0.0)
