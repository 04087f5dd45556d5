"""tests/area_shapes64.py, the float64 restatement of the area emitters' shapes, pinned on closed forms: the GPU tests lean on it, so it
must not lean on the GPU."""
import numpy as np

from tests import area_shapes64 as A


def midpoints(n):
    g = (np.arange(n) + 0.5) / n
    return np.stack(np.meshgrid(g, g, indexing="ij"), -1).reshape(-1, 2)


def test_cone_samples_lie_on_the_sphere_at_dist():
    sh = A.sphere([0.3, -0.2, 2.0], 0.7, [1, 1, 1])
    r = np.random.RandomState(1)
    ref = r.uniform(-1, 1, (4000, 3)) * [1.0, 1.0, 0.5]
    u = r.uniform(0, 1, (4000, 2))
    value, d, dist, pdf, n = A.sample_direct(sh, ref, u)
    p = ref + d * dist[:, None]
    assert np.max(np.abs(np.linalg.norm(p - sh.c, axis=1) - sh.R)) < 1e-9
    assert np.allclose(np.linalg.norm(d, axis=1), 1, atol=1e-12)
    assert np.allclose(n, (p - sh.c) / sh.R, atol=1e-7)                    # the outward normal at that point
    assert np.all((d * n).sum(1) < 0) and np.all(pdf > 0)                   # the near side faces the reference point
    # ... and the ray test finds the same point
    t = A.intersect(sh, ref, d)
    assert np.allclose(t, dist, rtol=0, atol=1e-7)


def test_cone_pdf_is_one_over_its_solid_angle():
    sh = A.sphere([0, 0, 0], 0.5, [2, 3, 4])
    r = np.random.RandomState(2)
    ref = r.normal(size=(1000, 3)); ref = ref / np.linalg.norm(ref, axis=1)[:, None] * r.uniform(0.6, 5.0, (1000, 1))
    u = r.uniform(0, 1, (1000, 2))
    value, d, dist, pdf, n = A.sample_direct(sh, ref, u)
    cosAlpha = np.sqrt(1 - (0.5 / np.linalg.norm(ref, axis=1)) ** 2)
    want = 1 / (2 * np.pi * (1 - cosAlpha))
    assert np.allclose(pdf, want, rtol=1e-12)
    assert np.allclose(A.pdf_direct(sh, ref, d, dist), want, rtol=1e-12)
    assert np.allclose(value, np.array([2, 3, 4]) / pdf[:, None], rtol=1e-12)


def sphere_irradiance(n, L, R, D):
    sh = A.sphere([0, 0, D], R, [L, L, L])
    u = midpoints(n)
    ref = np.zeros((u.shape[0], 3))
    value, d, dist, pdf, nn = A.sample_direct(sh, ref, u)
    return float(np.mean(value[:, 0] * d[:, 2]))                            # receiver at the origin facing the sphere (+z)


def test_sphere_irradiance_closed_form():
    L, R, D = 1.7, 0.8, 2.5
    tol = 1e-6
    e1, e2 = sphere_irradiance(32, L, R, D), sphere_irradiance(64, L, R, D)
    want = np.pi * L * (R / D) ** 2
    assert abs(e2 - e1) < tol * want                                        # the quadrature has converged below the tolerance it is held to
    assert abs(e2 - want) < tol * want


def disk_irradiance(n, L, r, h):
    m = np.eye(4); m[0, 0] = m[1, 1] = r; m[2, 2] = -1.0; m[2, 3] = h        # the disk at z = h facing down (negative determinant: flipped normal)
    sh = A.Shape(A.DISK, m, [L, L, L])
    assert np.allclose(sh.n, [0, 0, -1])
    u = midpoints(n)
    value, d, dist, pdf, nn = A.sample_direct(sh, np.zeros((u.shape[0], 3)), u)
    return float(np.mean(value[:, 0] * d[:, 2]))


def test_disk_on_axis_irradiance_closed_form():
    L, r, h = 0.9, 0.6, 1.1
    tol = 2e-5
    e1, e2 = disk_irradiance(128, L, r, h), disk_irradiance(256, L, r, h)
    want = np.pi * L * r * r / (h * h + r * r)
    assert abs(e2 - e1) < tol * want
    assert abs(e2 - want) < tol * want


def test_inside_branch_pdf_integrates_to_one():
    sh = A.sphere([0.1, 0.2, -0.1], 2.0, [1, 1, 1], flip=True)
    for ref in ([0.0, 0.0, 0.0], [0.9, -0.5, 0.7], [0.1, 0.2, -0.1]):
        totals = []
        for n in (128, 256):
            w = A.uniform_sphere(midpoints(n))                               # an equal-area grid of directions
            o = np.broadcast_to(np.asarray(ref, float), w.shape)
            t = A.intersect(sh, o, w)
            assert np.all(t > 0)
            pdf = A.pdf_direct(sh, o, w, t)
            assert np.all(pdf > 0)                                           # the flipped sphere faces every interior point
            totals.append(float(np.mean(pdf) * 4 * np.pi))
        assert abs(totals[1] - totals[0]) < 1e-5 and abs(totals[1] - 1) < 1e-5
    # and the sampler draws from that density: uniform by area
    u = midpoints(64)
    value, d, dist, pdf, n = A.sample_direct(sh, np.zeros((u.shape[0], 3)), u)
    assert np.allclose(pdf, A.pdf_direct(sh, np.zeros((u.shape[0], 3)), d, dist), rtol=1e-9)
    assert np.allclose(np.linalg.norm(d * dist[:, None] - sh.c, axis=1), sh.R, atol=1e-12)


def test_one_sided_radiance_and_planar_intersections():
    rect = A.Shape(A.RECT, np.diag([0.5, 0.25, 1.0, 1.0]), [1, 2, 3])
    disk = A.Shape(A.DISK, np.diag([0.5, 0.5, 1.0, 1.0]), [1, 2, 3])
    o = np.array([[0.4, 0.2, 1.0], [0.4, 0.3, 1.0], [0.4, 0.2, -1.0], [0.45, 0.24, 1.0]])
    down = np.array([[0, 0, -1.0]] * 4); down[2] = [0, 0, 1.0]
    assert list(A.intersect(rect, o, down)) == [1, -1, 1, 1]
    assert list(A.intersect(disk, o, down)) == [1, 1, 1, -1]                 # (0.45, 0.24) lies in the square's corner outside the disk
    p = o + down * 1.0
    assert np.all(A.radiance(rect, p, down)[0] == [1, 2, 3]) and np.all(A.radiance(rect, p, down)[2] == 0)   # from behind: black
    out = A.sphere([0, 0, 0], 1.0, [5, 5, 5]); inw = A.sphere([0, 0, 0], 1.0, [5, 5, 5], flip=True)
    o = np.array([[0, 0, 3.0], [0, 0, 0.5]]); d = np.array([[0, 0, -1.0], [0, 0, -1.0]])
    assert np.allclose(A.intersect(out, o, d), [2.0, 1.5])                   # the near root; from inside, the far one
    p = o + d * A.intersect(out, o, d)[:, None]
    assert list(A.radiance(out, p, d)[:, 0]) == [5, 0] and list(A.radiance(inw, p, d)[:, 0]) == [0, 5]
    assert A.intersect(out, o[:1], d[:1], 0.0, 1.5)[0] == -1 and A.intersect(out, o[1:], d[1:], 0.0, 1.0)[0] == -1
    idx, t = A.nearest([rect, out], np.array([[0.1, 0.1, 3.0]]), np.array([[0, 0, -1.0]]))
    assert idx[0] == 1 and abs(t[0] - (3 - np.sqrt(1 - 0.02))) < 1e-12
