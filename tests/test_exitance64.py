"""tests/exitance64.py, the float64 restatement of the exitance estimator (include/mer.h, mer_render_exitance), pinned by what an exitance
map must obey whatever the code: every escaping path lands in exactly one of sums / missed / rejected / late, the solid angles of the
cube's face cells seen from its centre, and Beer-Lambert on the cell under an unscattered beam.  tests/test_gpu_exitance.py holds the GPU
against the same closed forms and against this restatement.  No GPU, no library.

Set-up shared with the GPU tests: the cube [-1, 1]^3 (or the sphere of radius 1), the beam of power 5 from (0.2, 0.1, -3) along +z, maps
of 4 x 4 cells per face, K = 16 batches of 16 x 16 x 64 = 16 384 paths."""
import functools
import numpy as np
from tests import exitance64 as E

POWER = 5.0
BEAM = E.collimated([0.2, 0.1, -3.0], [0, 0, 1], POWER)
RES = (4, 4)
PATHS, K = 16 * 16 * 64, 16
SIGMA_S, SIGMA_A, G = 2.0, 0.2, 0.5
ABSORBER = 1.5                                 # sigma_a of the pure absorber
RADIUS = 1.0
# the beam's cell on face +z (face 5: axis 2, u = x, v = y): x = 0.2 -> iu 2, y = 0.1 -> iv 2
BEAM_FACE, BEAM_IV, BEAM_IU = 5, 2, 2
# the scene of the identity test: a beam that partly misses is not one ray, so a point emitter outside, close to the cube
OUTSIDE_POINT = E.point([0.0, 0.0, -1.5], 2.0)


@functools.lru_cache(maxsize=None)
def scattering_ref(shape_name):
    """the float64 reference of the scattering medium, computed once: (sums (K, 1, faces, 4, 4), totals (K, 16), exits per key)"""
    shape = E.CUBE if shape_name == "cube" else E.sphere(RADIUS)
    return E.render(BEAM, SIGMA_S, SIGMA_A, G, shape, RES, paths=PATHS, batches=K, seed=21 if shape_name == "cube" else 22, counts=True)


def test_every_escaping_path_lands_in_exactly_one_total():
    s, t = E.render(OUTSIDE_POINT, SIGMA_S, SIGMA_A, G, E.CUBE, RES, frames=8, t_min=0.5, t_bin=0.5, cos_min=0.5, n=1.33, paths=4096, batches=4, seed=1)
    assert np.all(t[:, 4] > 0) and np.all(t[:, 8] > 0) and np.all(t[:, 11] > 0) and s.sum() > 0
    assert E.identity_gap(s, t).max() < 1e-12
    # weight-1 settings: albedo 1 and depth below rr_depth: every exit weighs the power, so the count follows from the weights
    s, t = E.render(OUTSIDE_POINT, 2.0, 0.0, G, E.CUBE, RES, frames=8, t_min=0.5, t_bin=0.5, cos_min=0.5, paths=4096, batches=4, seed=2, rr_depth=10 ** 6)
    phi = OUTSIDE_POINT["phi"]
    np.testing.assert_allclose(t[:, 14], (t[:, 1] - t[:, 4] - t[:, 11] - t[:, 8]) / phi, rtol=1e-9)
    np.testing.assert_allclose(s.reshape(4, -1).sum(1), t[:, 14] * phi, rtol=1e-12)


def test_cube_cell_solid_angles():
    om = E.cube_cell_solid_angles(RES)
    assert om.shape == (4, 4) and np.all(om > 0)
    np.testing.assert_allclose(6 * om.sum(), 4 * np.pi, rtol=1e-14)
    np.testing.assert_allclose(om, om.T, rtol=1e-14); np.testing.assert_allclose(om, om[::-1, ::-1], rtol=1e-14)
    # a clear cube with a point emitter at its centre: every cell of every face holds I Omega per path, and nothing is lost
    em = E.point([0, 0, 0], 2.0)
    s, t = E.render(em, 0.0, 0.0, 0.0, E.CUBE, RES, paths=PATHS, batches=K, seed=3)
    ref = PATHS * 2.0 * np.broadcast_to(om, (6, 4, 4))
    p = np.broadcast_to(om, (6, 4, 4)) / (4 * np.pi)
    E.bar(s[:, 0].mean(0), np.sqrt(PATHS * em["phi"] ** 2 * p * (1 - p) / K), ref, what="clear cube cells")
    np.testing.assert_allclose(s.reshape(K, -1).sum(1), PATHS * em["phi"], rtol=1e-12)
    # the cone cos >= 0.8 about a face normal lies inside the face (tan = 0.75 < 1): 2 pi (1 - 0.8) I per face
    s, t = E.render(em, 0.0, 0.0, 0.0, E.CUBE, RES, cos_min=0.8, paths=PATHS, batches=K, seed=4)
    acc = 6 * 2 * np.pi * 0.2 * 2.0
    E.total_bar(s.reshape(K, -1).sum(1), PATHS * acc, what="accepted")
    E.total_bar(t[:, 11], PATHS * (em["phi"] - acc), what="rejected")
    assert E.identity_gap(s, t).max() < 1e-12


def test_beer_lambert_on_the_beams_cell():
    for n in (1.0, 1.4):
        s, t = E.render(BEAM, 0.0, ABSORBER, 0.0, E.CUBE, RES, n=n, paths=PATHS, batches=K, seed=5)
        on = np.zeros((6, 4, 4), bool); on[BEAM_FACE, BEAM_IV, BEAM_IU] = True
        assert np.all(s[:, 0][:, ~on] == 0.0)
        p = np.exp(-2 * ABSORBER)
        E.total_bar(s[:, 0, BEAM_FACE, BEAM_IV, BEAM_IU], PATHS * POWER * p, what="beam cell")
        # timed: the single frame that holds the exterior leg 2 + 2 n
        l = 2.0 + 2.0 * n
        s2, t2 = E.render(BEAM, 0.0, ABSORBER, 0.0, E.CUBE, RES, frames=8, t_min=2.25, t_bin=0.5, n=n, paths=PATHS, batches=2, seed=5)
        f = int(np.floor((l - 2.25) / 0.5))
        onf = np.zeros((8, 6, 4, 4), bool); onf[f, BEAM_FACE, BEAM_IV, BEAM_IU] = True
        assert np.all(s2[:, ~onf] == 0.0) and np.all(s2[:, onf] > 0) and np.all(t2[:, 8] == 0)


def test_sphere_cells_are_equal_area():
    em = E.point([0, 0, 0], 2.0)
    s, t = E.render(em, 0.0, ABSORBER, 0.0, E.sphere(RADIUS), RES, paths=PATHS, batches=K, seed=6)
    p = np.exp(-ABSORBER * RADIUS) / 16
    E.bar(s[:, 0, 0].mean(0), np.sqrt(PATHS * em["phi"] ** 2 * p * (1 - p) / K) * np.ones((4, 4)), PATHS * em["phi"] * p * np.ones((4, 4)), what="sphere cells")


def test_the_scattering_reference_fills_every_cell():
    """the condition of the GPU comparison: at these settings the reference alone puts at least 16 exits per batch into every cell of
    every face"""
    for name in ("cube", "sphere"):
        s, t, hits = scattering_ref(name)
        assert s.shape == (K, 1, 6 if name == "cube" else 1, 4, 4)
        print(name, "fewest exits in a cell of a batch:", hits.min())
        assert hits.min() >= 16, (name, hits.min())
        assert E.identity_gap(s, t).max() < 1e-12
