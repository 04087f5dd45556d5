"""tests/volpath64_all.py, the combined float64 reference of tests/test_gpu_combined.py, checked before it judges the HIP path: with every
feature but one switched off it is the single-feature volpath of that feature, so the two must agree on the same scene under the
acceptance rule of the GPU comparisons (tests/test_gpu_sensors.py: _agrees) -- 16 x 16 pixels, 2048 samples, independent streams."""
import numpy as np
import pytest
from mitsubaer_amd import params as P
from tests import sensors64 as S, volpath64_all as va, volpath64_multi as vm, volpath64_spot as vsp, volpath64_envmap as ve, volpath64_sensor as vse
from tests.envmap64 import EnvMap64, sun_and_gradient, rot
from tests.test_gpu_sensors import _agrees, _scaled

CAM = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
MED = (1.0, 0.5, 0.5)                                                           # sigma_s, sigma_a, g
VIEW = (16, 16, 50.0)
SPP = 2048
POINT = ([0.2, 0.3, -0.1], 3.0)
RECT = np.array([[0, 0, -1, -1.5], [0, 0.15, 0, 0.4], [0.15, 0, 0, 0.1]], np.float64)
RECT_ABOVE = np.array([[1.5, 0, 0, 0], [0, 0, -1, 2.5], [0, -1.5, 0, 0]], np.float64)
RECT_NEAR = np.array([[0.6, 0, 0, 0.8], [0, 0, -1, 1.6], [0, -0.6, 0, 0]], np.float64)
SPOT = np.array([[1.0, 0, 0, 0.3], [0, 0, -1, 0.6], [0, 1, 0, -0.2]])          # inside the cube, its axis along -y


def _st(m, v, ch=None):
    """(mean, variance of the mean) of one channel"""
    return (m, v / SPP) if ch is None else (m[..., ch], v[..., ch] / SPP)


def test_points_and_rectangles_alone_are_volpath64_multi():
    rects = lambda: [vm.Rect(RECT_ABOVE, 3.0), vm.Rect(RECT_NEAR, 1.5), vm.Rect(RECT, 4.0)]
    a = va.render(S.PERSPECTIVE, [POINT], [], rects(), 0.2, *MED, *VIEW, CAM, spp=SPP, seed=1)
    b = vm.render([POINT], rects(), 0.2, *MED, *VIEW, CAM, spp=SPP, seed=2)
    assert a[0].min() > 0 and np.array_equal(a[0][..., 0], a[0][..., 2])        # grey in, grey out
    assert _agrees(_st(*a, 0), _st(*b))


def test_points_and_spots_alone_are_volpath64_spot():
    spots = lambda: [vsp.Spot(SPOT, 5.0, 60.0), vsp.Spot(SPOT, 2.0, 20.0, 10.0)]
    a = va.render(S.PERSPECTIVE, [POINT], spots(), [], 0.2, *MED, *VIEW, CAM, spp=SPP, seed=3)
    b = vsp.render([POINT], spots(), 0.2, *MED, *VIEW, CAM, spp=SPP, seed=4)
    assert _agrees(_st(*a, 1), _st(*b))


def test_the_map_alone_is_volpath64_envmap():
    env = lambda: EnvMap64(sun_and_gradient(8, 16), rot([0.3, 1.0, -0.4], 57.0), 0.5)
    a = va.render(S.PERSPECTIVE, [], [], [], env(), *MED, *VIEW, CAM, spp=SPP, seed=5)
    b = ve.render(env(), *MED, *VIEW, CAM, spp=SPP, seed=6)
    for ch in range(3):
        assert _agrees(_st(*a, ch), _st(*b, ch))


@pytest.mark.parametrize("kind", [S.THINLENS, S.TELECENTRIC])
def test_a_lens_with_points_and_a_rectangle_is_volpath64_sensor(kind):
    cam = CAM if kind == S.THINLENS else _scaled(CAM, (1.3, 1.3, 1.0)).astype(np.float64)
    lens = dict(aperture_radius=0.3, focus_distance=3.0)
    a = va.render(kind, [POINT], [], [vm.Rect(RECT, 4.0)], 0.2, *MED, *VIEW, cam, spp=SPP, seed=7, **lens)
    b = vse.render(kind, [POINT], [vm.Rect(RECT, 4.0)], 0.2, *MED, *VIEW, cam, spp=SPP, seed=8, **lens)
    assert _agrees(_st(*a, 0), _st(*b))


def test_a_rectangle_that_does_not_block_the_luminaire_sample_changes_the_film():
    """the switch the GPU test turns off: with a rectangle over the map's bright patch, the estimator whose envmap samples ignore rectangles
    is a different (brighter) image"""
    img = np.full((8, 16, 3), 0.05, np.float32); img[0:2] = 30.0               # bright around +y only
    lid = lambda: [vm.Rect(np.array([[1.2, 0, 0, 0], [0, 0, -1, 1.5], [0, 1.2, 0, 0]], np.float64), 0.0)]
    a = va.render(S.PERSPECTIVE, [], [], lid(), EnvMap64(img), *MED, 8, 8, 50.0, CAM, spp=512, seed=9)
    b = va.render(S.PERSPECTIVE, [], [], lid(), EnvMap64(img), *MED, 8, 8, 50.0, CAM, spp=512, seed=9, env_sample_sees_rects=False)
    assert b[0].sum() > 1.5 * a[0].sum()
