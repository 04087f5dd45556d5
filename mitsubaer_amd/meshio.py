"""Triangle meshes for mer_sdf_from_mesh: a Wavefront OBJ reader and the library's refusals, without a GPU.

read_obj follows the rules of the host library's `obj` shape (mitsubaer_amd/host/mer_host.cpp): `v x y z` records and `f` records in the
forms i, i/j, i/j/k and i//k (only the vertex index is used), negative indices relative to the vertices read so far, polygons
triangulated as a fan around their first vertex.  Every other record is ignored.
"""
import numpy as np

MAX_TRIANGLES = 1 << 22


def read_obj(path):
    """-> (vertices float32 [V][3], triangles int32 [T][3])"""
    verts, tris = [], []
    with open(path, "r", errors="replace") as f:
        for line in f:
            tok = line.split("#", 1)[0].split()
            if not tok:
                continue
            if tok[0] == "v" and len(tok) >= 4:
                verts.append([float(tok[1]), float(tok[2]), float(tok[3])])
            elif tok[0] == "f":
                idx = []
                for t in tok[1:]:
                    i = int(t.split("/", 1)[0])
                    if i == 0:
                        raise ValueError("obj: face index 0 (indices start at 1)")
                    idx.append(i - 1 if i > 0 else len(verts) + i)
                for k in range(1, len(idx) - 1):
                    tris.append([idx[0], idx[k], idx[k + 1]])
    return np.asarray(verts, np.float32).reshape(-1, 3), np.asarray(tris, np.int32).reshape(-1, 3)


def degenerate(vertices, triangles):
    """bool [T]: a repeated index, or an exactly zero cross product (b - a) x (c - a) in float32 -- the triangles the library drops"""
    v = np.asarray(vertices, np.float32); t = np.asarray(triangles)
    a, b, c = v[t[:, 0]], v[t[:, 1]], v[t[:, 2]]
    e1, e2 = b - a, c - a
    n = np.stack([e1[:, 1] * e2[:, 2] - e1[:, 2] * e2[:, 1], e1[:, 2] * e2[:, 0] - e1[:, 0] * e2[:, 2], e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0]], 1)
    rep = (t[:, 0] == t[:, 1]) | (t[:, 1] == t[:, 2]) | (t[:, 0] == t[:, 2])
    return rep | (n == 0).all(1)


def validate(vertices, triangles):
    """The refusals of mer_sdf_from_mesh that concern the mesh, with its messages; -> (vertices float32 [V][3], triangles int32 [K][3]) with the
    degenerate triangles dropped, in their order."""
    v = np.ascontiguousarray(np.asarray(vertices, np.float32).reshape(-1, 3))
    t = np.ascontiguousarray(np.asarray(triangles, np.int64).reshape(-1, 3))
    if not 1 <= t.shape[0] <= MAX_TRIANGLES:
        raise ValueError("n_triangles must be in [1, 2^22]")
    if v.shape[0] < 1:
        raise ValueError("the mesh has no vertices")
    if (t < 0).any() or (t >= v.shape[0]).any():
        raise ValueError("triangle index out of range")
    if not np.isfinite(v).all():
        raise ValueError("a vertex is not finite")
    keep = ~degenerate(v, t)
    if not keep.any():
        raise ValueError("no triangle left after dropping the degenerate ones")
    return v, t[keep].astype(np.int32)
