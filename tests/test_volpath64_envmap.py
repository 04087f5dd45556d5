"""CPU checks of tests/volpath64_envmap.py, the float64 volpath the GPU envmap renders are held to per pixel: the furnace (a uniform map of
1 around a non-absorbing medium gives 1 everywhere) and a uniform map of c against the constant environment c of tests/volpath64_spot.py."""
import numpy as np
from mitsubaer_amd import params as P
from tests import volpath64_envmap as ve, volpath64_spot as vs
from tests.envmap64 import EnvMap64, rot

CAM = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])


def test_furnace():
    env = EnvMap64(np.ones((12, 20, 3), np.float32), rot([0.3, 1.0, -0.4], 57.0))
    m, v = ve.render(env, 1.0, 0.0, 0.5, 8, 8, 50.0, CAM, spp=512, seed=2)
    se = np.sqrt(v.mean() / 512)
    assert np.abs(m - 1).max() < 6 * np.sqrt(v.max() / 512) + 1e-9 and abs(m.mean() - 1) < 4 * se / 8 + 1e-3


def test_uniform_map_equals_the_constant_environment():
    c = [0.75, 0.375, 1.125]
    env = EnvMap64(np.broadcast_to(np.asarray(c, np.float32), (12, 20, 3)).copy(), rot([1.0, 0.2, 0.1], 33.0))
    m, v = ve.render(env, 1.0, 0.5, 0.5, 8, 8, 50.0, CAM, spp=1024, seed=3)
    for ch in range(3):
        r, rv = vs.render([], [], c[ch], 1.0, 0.5, 0.5, 8, 8, 50.0, CAM, spp=1024, seed=4)
        z = (m[..., ch] - r) / np.sqrt(v[..., ch] / 1024 + rv / 1024 + 1e-14)
        assert (np.abs(z) > 4).sum() <= 1, np.abs(z).max()
        assert abs(m[..., ch].mean() - r.mean()) < 4 * np.sqrt((v[..., ch].sum() + rv.sum()) / 1024) / 64
