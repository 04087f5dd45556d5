"""tests/volpath64_spot.py, the float64 reference of the spot-emitter GPU tests, checked before it judges the HIP path: its falloff against
values worked out by hand from spot.cpp:105-118, and a 180-degree spot against a point emitter at the same place."""
import numpy as np
from mitsubaer_amd import params as P
from tests import volpath64_spot as vs


def _dir_at(theta_deg):
    """the unit direction from a reference point to a spot at the origin whose axis is +z, the point lying theta off the axis"""
    t = np.radians(theta_deg)
    return -np.array([[np.sin(t), 0.0, np.cos(t)]])


def test_falloff_hand_values():
    s = vs.Spot(np.eye(4), 2.0, cutoff_deg=60.0, beam_deg=30.0)
    # inside the beam, on the ramp (halfway and a quarter of the way), on and past the cutoff, behind the emitter
    for theta, want in [(0.0, 1.0), (29.0, 1.0), (45.0, 0.5), (52.5, 0.25), (60.0 + 1e-9, 0.0), (75.0, 0.0), (180.0, 0.0)]:
        assert abs(s.falloff(_dir_at(theta))[0] - want) < 1e-9, (theta, s.falloff(_dir_at(theta)))
    # sampleDirect: I x falloff / dist^2 at distance 2 along 45 degrees
    ref = -2.0 * _dir_at(45.0)
    v, d, dist, f = s.sample_direct(ref)
    assert abs(dist[0] - 2.0) < 1e-12 and abs(f[0] - 0.5) < 1e-12 and abs(v[0] - 2.0 * 0.5 / 4.0) < 1e-12
    assert np.allclose(d, _dir_at(45.0))


def test_falloff_default_beam_and_scaled_frame():
    s = vs.Spot(np.eye(4), 1.0, cutoff_deg=20.0)          # beamWidth = 15 degrees
    assert abs(s.falloff(_dir_at(17.5))[0] - 0.5) < 1e-9
    # toWorld = scale(1, 1, 0.5): the z row of the inverse is (0, 0, 2), so cosTheta = 2 cos(theta) -- not a cosine (the reference's quirk).
    # theta = 70 degrees: cosTheta = 0.68404, acos = 46.84 degrees, falloff (60 - 46.84) / 30 = 0.4387
    s = vs.Spot(np.diag([1.0, 1.0, 0.5, 1.0]), 1.0, cutoff_deg=60.0, beam_deg=30.0)
    assert abs(s.falloff(_dir_at(70.0))[0] - (60.0 - np.degrees(np.arccos(2 * np.cos(np.radians(70.0))))) / 30.0) < 1e-9
    assert abs(s.falloff(_dir_at(70.0))[0] - 0.4387) < 1e-3
    assert s.falloff(_dir_at(50.0))[0] == 1.0                # 2 cos(50) > 1 >= cos(beam)
    # a rotated frame: axis along +x (rotate 90 degrees about y); a point at +x sees the full beam, one at +z sees none
    R = np.array([[0.0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 0]])
    s = vs.Spot(R, 1.0, cutoff_deg=30.0, beam_deg=10.0)
    assert s.falloff(np.array([[-1.0, 0, 0]]))[0] == 1.0 and s.falloff(np.array([[0, 0, -1.0]]))[0] == 0.0


def test_180_degree_spot_is_a_point():
    cam = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
    pos = [-1.6, 1.4, 0.4]
    M = np.array([[1.0, 0, 0, pos[0]], [0, 0, -1, pos[1]], [0, 1, 0, pos[2]]])
    a, va = vs.render([(pos, 3.0)], [], 0.2, 1.0, 0.5, 0.5, 4, 4, 30.0, cam, spp=64, seed=7)
    b, vb = vs.render([], [vs.Spot(M, 3.0, 180.0, 180.0)], 0.2, 1.0, 0.5, 0.5, 4, 4, 30.0, cam, spp=64, seed=7)
    assert a.min() > 0
    np.testing.assert_allclose(a, b, rtol=1e-12)


def test_spot_lights_only_its_cone():
    """a narrow spot above the cube aimed straight down lights the centre of the image far more than an equally bright one aimed away"""
    cam = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
    down = np.array([[1.0, 0, 0, 0], [0, 0, -1, 2.5], [0, 1, 0, 0]])      # z axis -> -y
    up = np.array([[1.0, 0, 0, 0], [0, 0, 1, 2.5], [0, -1, 0, 0]])       # z axis -> +y
    a, _ = vs.render([], [vs.Spot(down, 5.0, 15.0, 10.0)], 0.0, 1.0, 0.5, 0.5, 8, 8, 30.0, cam, spp=64, seed=8)
    b, _ = vs.render([], [vs.Spot(up, 5.0, 15.0, 10.0)], 0.0, 1.0, 0.5, 0.5, 8, 8, 30.0, cam, spp=64, seed=8)
    assert a[3:5, 3:5].mean() > 0 and (b == 0).all()
