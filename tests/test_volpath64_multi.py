"""tests/volpath64_multi.py, the float64 reference of the multi-emitter GPU test, proven on a closed form before it judges the HIP path: in a
non-absorbing medium lit only by an environment of radiance 1 every pixel's expectation is 1 (its environment sample and look-up, with their
MIS weights, add up to the whole environment), and rectangles that are not there change nothing."""
import numpy as np
from mitsubaer_amd import params as P
from tests import volpath64_multi as vm


def test_furnace():
    cam = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
    S = 2048
    m, v = vm.render([], [], 1.0, 1.0, 0.0, 0.5, 4, 4, 30.0, cam, spp=S, seed=3)
    assert abs(m.mean() - 1.0) < 4 * np.sqrt(v.sum() / S) / m.size
    z = (m - 1.0) / np.sqrt(v / S + 1e-14)
    assert (np.abs(z) < 4.5).all(), z


def test_hidden_rectangle_contributes_nothing():
    """a bright rectangle above the cube behind a black one that covers every line of sight to it: the image is exactly zero, while the
    bright one alone lights it"""
    cam = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
    bright = vm.Rect([[1.5, 0, 0, 0], [0, 0, -1, 2.5], [0, -1.5, 0, 0]], 3.0)
    black = vm.Rect([[3.0, 0, 0, 0], [0, 0, -1, 1.5], [0, -3.0, 0, 0]], 0.0)
    m, _ = vm.render([], [bright, black], 0.0, 1.0, 0.5, 0.5, 4, 4, 30.0, cam, spp=128, seed=4)
    assert (m == 0).all()
    m, _ = vm.render([], [bright], 0.0, 1.0, 0.5, 0.5, 4, 4, 30.0, cam, spp=128, seed=4)
    assert (m > 0).all()
