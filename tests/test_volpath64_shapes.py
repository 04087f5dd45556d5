"""tests/volpath64_shapes.py, the float64 volpath the GPU renders of sphere / disk / rectangle area emitters are held to, checked on its
own: a furnace whose answer is known, and two seeds of the reference pass against each other by the GPU test's own z-test."""
import numpy as np

from mitsubaer_amd import params as P
from tests import volpath64_shapes as vs


def test_furnace_inside_a_flipped_sphere():
    """albedo 1, an inward-facing sphere of radiance 1 around cube and camera, no environment: every path carries radiance 1 in
    expectation, whatever it does in the medium"""
    cam = P.look_at([-1.8, 0.2, 0.1], [0, 0, 0], [0, 1, 0])
    spp = 256
    m, v = vs.render([vs.Sphere([0.1, -0.1, 0.2], 3.0, 1.0, flip=True)], 0.0, 1.0, 0.0, 0.6, 8, 8, 70.0, cam, spp=spp, seed=3, max_bounces=2000)
    se = np.sqrt(v.mean() / (m.size * spp))
    assert v.max() > 0                                                       # not only pixels that see the sphere directly
    assert abs(m.mean() - 1) < 4 * se, (m.mean(), se)


def test_two_seeds_of_the_mixed_scene_agree():
    """the z-test tests/test_gpu_area_shapes.py applies to the GPU, applied to two seeds of the reference itself: at most 1 + 1 % of the 256
    pixels beyond 4 sigma and the image total within 4 sigma.  Observed: 0 outliers; totals differ by 0.145 against a bound of 0.326."""
    m1, v1 = vs.mixed_reference(1)
    m2, v2 = vs.mixed_reference(2)
    S = vs.MIXED_SPP
    outliers, allowed, dtot, bound = vs.z_test(m1, v1, S, m2, v2, S)
    print("outliers %d (allowed %.2f), totals differ by %.4f (4 sigma = %.4f)" % (outliers, allowed, dtot, bound))
    assert outliers <= allowed
    assert abs(dtot) < bound
    assert m1.mean() > 0.1 and m1.max() == 3.0                               # lit, and some pixel looks straight at the sphere
