"""The features of the EXTRA kernels TOGETHER, per pixel against one float64 volpath (tests/volpath64_all.py): a lens or parallel sensor, an
emitter list that mixes points, spots and rectangles with unequal sampling weights, and an environment map -- the interactions include/mer.h
writes down under n_emitters and that no single-feature volpath reaches.  Each scene must agree with the combined reference under the
acceptance rule of tests/test_gpu_sensors.py (at most 1 + 1 % of the pixels beyond 4 sigma, the image total within 4 sigma; red channel, 32
batches of 64 samples against 2048 float64 samples) and must DISAGREE with the same reference computed with one interaction removed.  The two
float64 films of every scene differ by that rule themselves (outliers of 256, first with the interaction, i.e. two independent runs of the
right reference, then right against wrong):
  1. lens_map_spot_point_rect   the rectangle does not block the map's luminaire samples        0 and 158
  2. lens_two_rects_two_spots   only the first entry of the point table is ever sampled          0 and 43
  3. parallel_map_points        the map is not rotated                                           0 and 138"""
import numpy as np
import pytest
from tests import volpath64_all as va
from tests.combined_scenes import MED64, NAMES, scene as _scene
from tests.test_gpu_sensors import _agrees, _stats

pytestmark = pytest.mark.gpu

SPP = 2048


def reference(args, seed):
    """(mean, variance of the mean) of the red channel of the float64 film"""
    a = dict(args)
    m, v = va.render(a.pop("kind"), a.pop("points"), a.pop("spots"), a.pop("rects"), a.pop("env"), *MED64, 16, 16, 50.0, np.asarray(a.pop("cam_to_world"), np.float64),
                     spp=SPP, seed=seed, **a)
    return m[..., 0], v[..., 0] / SPP


@pytest.mark.parametrize("name", NAMES)
def test_combined_scene_matches_the_float64_volpath(ctx, name):
    p, right, wrong = _scene(name)
    ref = reference(right, 1)
    other = reference(wrong, 2)
    assert ref[0].mean() > 0.1
    assert not _agrees(ref, other)                                             # the two float64 films differ: the scene sees the interaction
    gpu = _stats(ctx, p, B=32, spp=64, seed=11)
    ok = _agrees(gpu, ref)
    bad = _agrees(gpu, other)
    assert ok and not bad
