"""tests/sensors64.py, the float64 restatement the GPU sensor tests compare with, checked on properties that need no renderer."""
import numpy as np
import pytest
from mitsubaer_amd import params as P
from tests import ref64, sensors64 as S

W, H, FOV, NEAR, FAR = 12, 8, 40.0, 0.05, 50.0


def _to_world(scale=(1.0, 1.0, 1.0)):
    m = np.asarray(P.look_at([-3, 0.2, 0.1], [-2, 0.1, 0.3], [0, 1, 0]), np.float64).copy()
    m[:3, :3] = m[:3, :3] * np.asarray(scale, np.float64)[None, :]         # toWorld = lookAt * scale(s): the columns are scaled
    return m


def _positions():
    xs = np.concatenate([np.arange(W + 1), np.arange(W) + 0.5]); ys = np.concatenate([np.arange(H + 1), np.arange(H) + 0.5])
    X, Y = np.meshgrid(xs, ys)
    return np.stack([X.ravel(), Y.ravel()], 1)


def test_perspective_is_the_pinhole_of_ref64():
    T = _to_world(); pos = _positions()
    o, d, mint, maxt = S.sensor_rays(S.PERSPECTIVE, T, W, H, FOV, NEAR, FAR, pos)
    ro, rd = ref64.pinhole_rays(T, W, H, FOV, pos)
    assert np.abs(o - ro).max() < 1e-14 and np.abs(d - rd).max() < 1e-14
    cz = d @ T[:3, 2]                                                      # cosine to the optical axis: the clip planes are z = near, z = far
    assert np.allclose(mint * cz, NEAR, rtol=1e-6) and np.allclose(maxt * cz, FAR, rtol=1e-6)    # look_at is a float32 matrix


def test_orthographic_rays_are_parallel_and_tile_the_sensor_rectangle():
    sc = (1.5, 0.75, 2.0)
    T = _to_world(sc); pos = _positions()
    o, d, mint, maxt = S.sensor_rays(S.ORTHOGRAPHIC, T, W, H, FOV, NEAR, FAR, pos)
    axis = T[:3, 2] / np.linalg.norm(T[:3, 2])
    assert np.abs(d - axis).max() < 1e-15
    assert np.all(mint == NEAR) and np.all(maxt == FAR)                    # not rescaled by |T e_z|: the reference's quirk
    # back to camera space: the origins are (1 - 2 sx, (1 - 2 sy) / aspect, 0), i.e. they tile [-1, 1] x [-1 / aspect, 1 / aspect]
    q = np.linalg.solve(T[:3, :3], (o - T[:3, 3]).T).T
    aspect = W / H
    assert np.abs(q[:, 2]).max() < 1e-14
    assert np.abs(q[:, 0] - (1 - 2 * pos[:, 0] / W)).max() < 1e-14 and np.abs(q[:, 1] - (1 - 2 * pos[:, 1] / H) / aspect).max() < 1e-14
    assert np.isclose(q[:, 0].min(), -1) and np.isclose(q[:, 0].max(), 1) and np.isclose(q[:, 1].min(), -1 / aspect) and np.isclose(q[:, 1].max(), 1 / aspect)
    corner = S.sensor_rays(S.ORTHOGRAPHIC, T, W, H, FOV, NEAR, FAR, [[0.0, 0.0]])[0][0]
    assert np.allclose(corner, T[:3, 3] + T[:3, 0] + T[:3, 1] / aspect)   # the film's first corner is +x, +y of the camera


@pytest.mark.parametrize("kind, scale", [(S.THINLENS, (1, 1, 1)), (S.TELECENTRIC, (1.5, 0.75, 2.0))])
def test_every_aperture_sample_of_a_pixel_meets_the_focal_plane_in_one_point(kind, scale):
    T = _to_world(scale); focus, radius = 2.75, 0.4
    rng = np.random.default_rng(3)
    u = np.concatenate([rng.random((61, 2)), [[0.5, 0.5], [0.0, 0.0], [1.0, 1.0]]])
    A = T[:3, :3]; lens = np.linalg.norm(A, axis=0)
    zf = focus if kind == S.THINLENS else focus / lens[2]
    for px in ([0.0, 0.0], [3.25, 6.5], [W, H], [W / 2, H / 2]):
        pos = np.tile(px, (len(u), 1))
        o, d, _, _ = S.sensor_rays(kind, T, W, H, FOV, NEAR, FAR, pos, u, radius, focus)
        oc = np.linalg.solve(A, (o - T[:3, 3]).T).T; dc = np.linalg.solve(A, d.T).T     # camera space
        hit = oc + dc * ((zf - oc[:, 2]) / dc[:, 2])[:, None]
        assert np.abs(hit - hit[0]).max() < 1e-12
        x, y = S.near_plane(kind, W, H, FOV, pos[:1])
        want = [x[0] * zf, y[0] * zf, zf] if kind == S.THINLENS else [x[0], y[0], zf]
        assert np.abs(hit[0] - want).max() < 1e-12
        # the origins fill the aperture: within its radius around the lens centre (thin lens) / the pixel's own origin (telecentric)
        centre = np.zeros(3) if kind == S.THINLENS else np.array([x[0], y[0], 0.0])
        rad = np.linalg.norm(oc - centre, axis=1)
        assert rad.max() <= (radius if kind == S.THINLENS else radius / lens[0]) * (1 + 1e-12) and np.abs(oc[:, 2]).max() < 1e-14


def test_thin_lens_tends_to_the_pinhole_and_telecentric_to_orthographic():
    T = _to_world(); pos = _positions()
    u = np.random.default_rng(5).random((len(pos), 2))
    po, pd, pmin, pmax = S.sensor_rays(S.PERSPECTIVE, T, W, H, FOV, NEAR, FAR, pos)
    err = []
    for radius in (1e-2, 1e-4, 1e-6):
        o, d, mint, maxt = S.sensor_rays(S.THINLENS, T, W, H, FOV, NEAR, FAR, pos, u, radius, 4.0)
        err.append(max(np.abs(o - po).max(), np.abs(d - pd).max(), np.abs(mint / pmin - 1).max()))
        assert err[-1] <= radius * 1.0001
    assert err[0] > err[1] > err[2]
    Ts = _to_world((1.5, 0.75, 2.0))
    oo, od, _, _ = S.sensor_rays(S.ORTHOGRAPHIC, Ts, W, H, FOV, NEAR, FAR, pos)
    o, d, mint, maxt = S.sensor_rays(S.TELECENTRIC, Ts, W, H, FOV, NEAR, FAR, pos, u, 0.0, 4.0)
    assert np.abs(o - oo).max() < 1e-15 and np.abs(d - od).max() < 1e-15 and np.all(mint == NEAR) and np.all(maxt == FAR)


def test_concentric_disk_map_is_area_preserving():
    n = 1 << 22
    p = S.concentric_disk(np.random.default_rng(11).random((n, 2)))
    r = np.linalg.norm(p, axis=1); phi = np.arctan2(p[:, 1], p[:, 0])
    assert r.max() <= 1.0
    # equal-area bins of the disk: 8 rings of equal area x 16 sectors; a uniform sample puts Binomial(n, 1/128) points in each
    ring = np.minimum((r * r * 8).astype(int), 7); sector = np.minimum(((phi + np.pi) / (2 * np.pi) * 16).astype(int), 15)
    counts = np.bincount(ring * 16 + sector, minlength=128)
    sigma = np.sqrt(n / 128 * (1 - 1 / 128))
    assert np.abs(counts - n / 128).max() < 5 * sigma, (np.abs(counts - n / 128).max() / sigma)     # 5 sigma: 0.55 % of a bin
    # branch boundaries and the centre
    q = S.concentric_disk([[0.5, 0.5], [1.0, 0.5], [0.5, 1.0], [0.0, 0.5], [0.5, 0.0], [1.0, 1.0], [0.0, 0.0], [0.75, 0.75]])
    s = np.sqrt(0.5)
    want = [[0, 0], [1, 0], [0, 1], [-1, 0], [0, -1], [s, s], [-s, -s], [0.5 * s, 0.5 * s]]
    assert np.abs(q - want).max() < 1e-15


def test_volpath64_sensor_swaps_the_ray_generator_and_restores_it():
    """tests/volpath64_sensor.py: an orthographic view 6 wide sees the environment exactly in the pixels whose rays pass beside the cube, and a
    darker value through it; volpath64_multi keeps its own ray generator afterwards"""
    from tests import volpath64_multi as vm, volpath64_sensor as vs
    T = np.asarray(P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0]), np.float64).copy()
    T[:3, :3] = T[:3, :3] * np.array([3.0, 3.0, 1.0])[None, :]
    m, v = vs.render(S.ORTHOGRAPHIC, [], [], 0.5, 1.0, 1.0, 0.0, 6, 6, 50.0, T, spp=64, seed=1)
    assert vm.ref64 is ref64
    beside = np.ones((6, 6), bool); beside[2:4, 2:4] = False                # the cube's silhouette [-1, 1]^2 is the central 2 x 2 pixels
    assert np.all(m[beside] == 0.5) and np.all(v[beside] == 0)
    assert np.all(m[~beside] < 0.45) and np.all(m[~beside] > 0.0)
    # a telecentric lens focused on the cube's far side blurs the silhouette: the pixels next to it are no longer pure environment
    m2, _ = vs.render(S.TELECENTRIC, [], [], 0.5, 1.0, 1.0, 0.0, 6, 6, 50.0, T, aperture_radius=0.6, focus_distance=6.0, spp=64, seed=1)
    assert np.any(m2[1, 2:4] < 0.5) and np.all(m2[0, :] == 0.5)
