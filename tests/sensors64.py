"""Float64 restatement of the primary rays of the four projective sensors (src/sensors/perspective.cpp:247-269,
orthographic.cpp:107-155, thinlens.cpp:293-322, telecentric.cpp:140-222) and of warp::squareToUniformDiskConcentric (src/libcore/warp.cpp:
81-100), written from their definitions and independent of the HIP code.

px, py are film coordinates in pixels; sx = px / W, sy = py / H, aspect = W / H; T is the sensor's toWorld (3x4 or 4x4); u is the aperture
sample in [0, 1)^2.
  perspective   nearP = (tan(fov_x/2) (1 - 2 sx), tan(fov_x/2) (1 - 2 sy) / aspect, 1) near; d = T normalize(nearP), o = T (0, 0, 0),
                mint = near / dl.z, maxt = far / dl.z
  orthographic  nearP = (1 - 2 sx, (1 - 2 sy) / aspect): the inverse of scale(-1/2, -aspect/2, 1) translate(-1, -1/aspect, 0) orthographic(near, far)
                o = T (nearP.x, nearP.y, 0), d = normalize(T (0, 0, 1)), mint = near, maxt = far
  thinlens      apertureP = disk(u) R, focusP = nearP (focus / nearP.z), dl = normalize(focusP - apertureP); o = T apertureP, d = T dl,
                mint = near / dl.z, maxt = far / dl.z
  telecentric   scale = the lengths of T's columns; disk = disk(u) R / scale.x; focusP = (orthographic nearP.xy, focus / scale.z);
                orig = (disk + focusP.xy, 0); o = T orig, d = normalize(T (focusP - orig)), mint = near, maxt = far
"""
import numpy as np

PERSPECTIVE, ORTHOGRAPHIC, THINLENS, TELECENTRIC = 0, 1, 2, 3
KINDS = {"perspective": PERSPECTIVE, "orthographic": ORTHOGRAPHIC, "thinlens": THINLENS, "telecentric": TELECENTRIC}


def concentric_disk(u):
    """squareToUniformDiskConcentric: u [n, 2] in [0, 1]^2 -> points of the unit disk [n, 2]"""
    u = np.asarray(u, np.float64)
    r1 = 2 * u[:, 0] - 1; r2 = 2 * u[:, 1] - 1
    first = r1 * r1 > r2 * r2
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(first, r1, r2)
        phi = np.where(first, (np.pi / 4) * (r2 / r1), np.pi / 2 - (r1 / r2) * (np.pi / 4))
    zero = (r1 == 0) & (r2 == 0)
    r = np.where(zero, 0.0, r); phi = np.where(zero, 0.0, phi)
    return np.stack([r * np.cos(phi), r * np.sin(phi)], 1)


def _matrix(to_world):
    M = np.eye(4); t = np.asarray(to_world, np.float64); M[:t.shape[0], :4] = t
    return M[:3, :3], M[:3, 3]


def near_plane(kind, width, height, fov_x_deg, pos):
    """camera-space (x, y) of the film position on the plane z = 1 (perspective kinds) or on the sensor plane (parallel kinds)"""
    pos = np.asarray(pos, np.float64)
    sx = pos[:, 0] / width; sy = pos[:, 1] / height; aspect = width / height
    x = 1 - 2 * sx; y = (1 - 2 * sy) / aspect
    if kind in (PERSPECTIVE, THINLENS):
        t = np.tan(np.deg2rad(fov_x_deg) / 2)
        return x * t, y * t
    return x, y


def camera_rays(kind, width, height, fov_x_deg, near, far, pos, u=None, aperture_radius=0.0, focus_distance=1.0, scale=(1.0, 1.0, 1.0)):
    """the ray in CAMERA space: origin [n, 3], direction [n, 3] (unit for every kind but telecentric, whose world direction is
    normalised after the transform), mint, maxt [n] (the parallel kinds': valid once the world direction is normalised)"""
    pos = np.asarray(pos, np.float64); n = len(pos)
    x, y = near_plane(kind, width, height, fov_x_deg, pos)
    if kind in (THINLENS, TELECENTRIC):
        disk = concentric_disk(u)
    if kind == PERSPECTIVE or kind == THINLENS:
        nearP = np.stack([x * near, y * near, np.full(n, float(near))], 1)
        if kind == PERSPECTIVE:
            org = np.zeros((n, 3)); dl = nearP
        else:
            org = np.concatenate([disk * aperture_radius, np.zeros((n, 1))], 1)
            dl = nearP * (focus_distance / nearP[:, 2:3]) - org
        dl = dl / np.linalg.norm(dl, axis=1, keepdims=True)
        return org, dl, near / dl[:, 2], far / dl[:, 2]
    if kind == ORTHOGRAPHIC:
        org = np.stack([x, y, np.zeros(n)], 1); dl = np.tile([0.0, 0.0, 1.0], (n, 1))
    else:
        disk = disk * (aperture_radius / scale[0])
        focusP = np.stack([x, y, np.full(n, focus_distance / scale[2])], 1)
        org = np.stack([disk[:, 0] + x, disk[:, 1] + y, np.zeros(n)], 1)
        dl = focusP - org
    return org, dl, np.full(n, float(near)), np.full(n, float(far))


def sensor_rays(kind, to_world, width, height, fov_x_deg, near, far, pos, u=None, aperture_radius=0.0, focus_distance=1.0):
    """world rays: o [n, 3], d [n, 3], mint [n], maxt [n]"""
    A, t = _matrix(to_world)
    scale = np.linalg.norm(A, axis=0)
    org, dl, mint, maxt = camera_rays(kind, width, height, fov_x_deg, near, far, pos, u, aperture_radius, focus_distance, scale)
    o = org @ A.T + t
    d = dl @ A.T
    if kind in (ORTHOGRAPHIC, TELECENTRIC):
        d = d / np.linalg.norm(d, axis=1, keepdims=True)
    return o, d, mint, maxt
