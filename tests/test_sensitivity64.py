"""tests/sensitivity64.py, the float64 restatement of the sensitivity grid (mer_render_sensitivity), against three closed forms.  No GPU.

Set-up: the cube [-1, 1]^3, the beam of power (5, 3, 8) from (0.25, 0.25, -3) along +z, grids of 4^3 cells over the cube, the detector a
window of a 4 x 4 raster on face 5 (z = +1).  The beam meets raster cell (iu, iv) = (2, 2) and grid column ix = iy = 2."""
import numpy as np
from tests import sensitivity64 as S

POWER3 = np.array([5.0, 3.0, 8.0])
BEAM = S.collimated([0.25, 0.25, -3.0], [0, 0, 1], 1.0)
RES = (4, 4, 4)
BEAM_CELL = S.detector((4, 4), 5, (2, 3, 2, 3))
PATHS = 4096
ABSORBER = 0.8
# the derivative test's medium: manual sampling at a fixed density, the roulette out of reach, at most 20 flights of at most 2 sqrt(3) each
DERIV = dict(sigma_s=np.array([1.2, 0.9, 1.5]), sigma_a=np.array([0.30, 0.45, 0.20]), density=1.1, weight=0.8, g=0.5, delta=1e-3,
             rr_depth=100000, max_depth=20, det=S.detector((4, 4), 5, (1, 3, 1, 3), cos_min=0.2))
DERIV_RTOL = 2e-3       # per path W(s +- delta) = w exp(-+ delta L): the central difference is w L (1 + delta^2 L^2 / 6 + ...), and L <= 20 x 2 sqrt(3) < 70: at most 8.2e-4


def column(j):
    on = np.zeros(j.shape[1:4], bool); on[:, 2, 2] = True
    return on


def test_clear_cube_column():
    """no extinction: every path is detected with w = P and flew the beam's column: J_c = paths P 2 / nz there, exactly 0 elsewhere"""
    j, t = S.render(BEAM, POWER3, S.LP.homogeneous(0.0, 0.0, "single"), 0.0, RES, BEAM_CELL, paths=PATHS, batches=2)
    on = column(j)
    assert np.all(j[:, ~on] == 0.0)
    np.testing.assert_allclose(j[:, on], np.broadcast_to(PATHS * POWER3 * 0.5, (2, 4, 3)), rtol=1e-12, atol=0)
    assert np.all(t[:, 8] == PATHS) and np.all(t[:, 0] == PATHS) and np.all(t[:, 4:7] == 0)
    np.testing.assert_allclose(t[:, 1:4], np.broadcast_to(PATHS * POWER3, (2, 3)), rtol=1e-12, atol=0)
    np.testing.assert_allclose(t[:, 9:12], np.broadcast_to(PATHS * POWER3 * 2.0, (2, 3)), rtol=1e-12, atol=0)
    # a window beside the beam's cell detects nothing
    j0, t0 = S.render(BEAM, POWER3, S.LP.homogeneous(0.0, 0.0, "single"), 0.0, RES, S.detector((4, 4), 5, (0, 2, 0, 4)), paths=256, batches=1)
    assert not j0.any() and t0[0, 8] == 0 and not t0[0, 1:13].any()


def test_pure_absorber_column():
    """sigma_s = 0: a path is detected iff its first flight passes the cube, with w = P exactly (transmittance / pdfFailure = 1 under analog
    sampling): J_c = detected P 2 / nz given the detected count, which is binomial with p = exp(-2 sigma_t)"""
    k = 8
    j, t = S.render(BEAM, POWER3, S.LP.homogeneous(0.0, ABSORBER, "single"), 0.0, RES, BEAM_CELL, paths=PATHS, batches=k, seed=3)
    on = column(j)
    assert np.all(j[:, ~on] == 0.0)
    for b in range(k):
        np.testing.assert_allclose(j[b][on], np.broadcast_to(t[b, 8] * POWER3 * 0.5, (4, 3)), rtol=1e-12, atol=0)
    p = np.exp(-2 * ABSORBER)
    z = abs(t[:, 8].sum() - k * PATHS * p) / np.sqrt(k * PATHS * p * (1 - p))
    print("detected %d of %d, expected %.1f, z %.2f" % (t[:, 8].sum(), k * PATHS, k * PATHS * p, z))
    assert z <= 4 and 0 < t[:, 8].min() and t[:, 8].max() < PATHS


def deriv_signal(sigma_a_shift, seed=5, paths=PATHS):
    m = S.manual(DERIV["sigma_s"], DERIV["sigma_a"] + sigma_a_shift, DERIV["density"], DERIV["weight"])
    return S.render(BEAM, POWER3, m, DERIV["g"], RES, DERIV["det"], paths=paths, batches=1, seed=seed, rr_depth=DERIV["rr_depth"], max_depth=DERIV["max_depth"])


def test_jacobian_is_minus_the_derivative_of_the_signal():
    """the walks at sigma_a +- delta are the same paths (fixed density, no roulette): the central difference of W_det equals -sum(J)"""
    d = DERIV["delta"]
    j, t = deriv_signal(0.0)
    _, tp = deriv_signal(+d)
    _, tm = deriv_signal(-d)
    assert tp[0, 8] == tm[0, 8] == t[0, 8] and 0 < t[0, 8] < PATHS            # the same paths, some detected and some not
    diff = (tp[0, 1:4] - tm[0, 1:4]) / (2 * d)
    jsum = j[0].reshape(-1, 3).sum(0)
    print("dW/dsigma_a", diff, "-sum(J)", -jsum, "ratio", diff / -jsum)
    np.testing.assert_allclose(diff, -jsum, rtol=DERIV_RTOL, atol=0)
    # the box is the cube: nothing is dropped, and the cells hold all of the paths' length
    assert not t[0, 4:7].any()
    np.testing.assert_allclose(jsum, t[0, 9:12], rtol=1e-12, atol=0)
    lbar = t[0, 9:12] / t[0, 1:4]
    assert np.all(lbar >= 2.0) and np.all(lbar < 70.0)                          # the mean path length of the detected light
