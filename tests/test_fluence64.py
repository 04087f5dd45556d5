"""tests/fluence64.py, the float64 restatement of the fluence estimator (include/mer.h, mer_render_fluence), pinned by what a fluence grid
must obey whatever the code: Beer-Lambert along an unscattered beam, exact zeros off the beam, and the energy balance -- absorbed plus
escaped (plus what fell outside the box) equals emitted.  tests/test_gpu_fluence.py holds the GPU against the same closed forms and
against this restatement.  No GPU, no library.

Set-up shared with the GPU tests: the cube [-1, 1]^3, the beam of power 5 from (0.2, 0.1, -3) along +z, an 8 x 8 x 8 grid over the cube,
K = 16 batches of 16 x 16 x 64 = 16 384 paths (a dim cell of the scattering medium is hit in only ~11 of 16 batches of 4 096 paths: its
batch spread is not Gaussian there)."""
import numpy as np
from tests import fluence64 as F

POWER = 5.0
BEAM = F.collimated([0.2, 0.1, -3.0], [0, 0, 1], POWER)
RES = (8, 8, 8)
PATHS, K = 16 * 16 * 64, 16
SIGMA_S, SIGMA_A, G = 2.0, 0.25, 0.6
ABSORBER = 1.5                                 # sigma_a of the pure absorber
CUT = dict(res=(4, 6, 5), bmin=(-1.0, -0.5, -1.0), bmax=(0.5, 1.0, 0.25))       # a box that cuts the cube


def column_check(sums, sigma_t, paths, what, res=RES, bmin=(-1, -1, -1), bmax=(1, 1, 1)):
    """(batches, nz, ny, nx) raw sums of FIRST collisions of the beam against Beer-Lambert: the column within the bar under the binomial
    variance, every other cell exactly 0"""
    p = F.beam_column(BEAM, sigma_t, res, bmin, bmax)
    k = len(sums)
    ref = paths * POWER / sigma_t * p
    sd = np.sqrt(paths * (POWER / sigma_t) ** 2 * p * (1 - p) / k)
    on = p > 0
    assert on.any()
    assert np.all(sums[:, ~on] == 0.0), "deposits off the beam's column"
    F.bar(sums.mean(0)[on], sd[on], ref[on], what=what)


def test_pure_absorber_is_beer_lambert():
    sums, tot = F.render(BEAM, 0.0, ABSORBER, 0.0, RES, paths=PATHS, batches=K, seed=1)
    column_check(sums, ABSORBER, PATHS, "absorber column")
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:] == 0)
    # escaped: paths x P e^{-2 sigma} (binomial)
    pe = np.exp(-2 * ABSORBER)
    F.total_bar(tot[:, 1], PATHS * POWER * pe, what="absorber escaped")
    bal = ABSORBER * sums.sum((1, 2, 3)) + tot[:, 1]
    np.testing.assert_allclose(bal, PATHS * POWER, rtol=1e-12)          # every path deposits P / sigma once or escapes with P


def test_energy_balance_of_a_scattering_medium():
    sums, tot = F.render(BEAM, SIGMA_S, SIGMA_A, G, RES, paths=PATHS, batches=K, seed=2)
    assert np.all(tot[:, 4:] == 0)
    bal = SIGMA_A * sums.sum((1, 2, 3)) + tot[:, 1]
    F.total_bar(bal, PATHS * POWER, what="balance")
    assert abs(bal.mean() / (PATHS * POWER) - 1) < 5e-3
    # the restatement against itself, another seed: per cell within the bar with both batch spreads
    s2, _ = F.render(BEAM, SIGMA_S, SIGMA_A, G, RES, paths=PATHS, batches=K, seed=3)
    F.bar(sums.mean(0), sums.std(0, ddof=1) / np.sqrt(K), s2.mean(0), s2.var(0, ddof=1) / K, what="self")
    assert (sums.mean(0) > 0).all()                                        # light reaches every cell


def test_max_depth_2_keeps_the_first_collisions():
    sums, tot = F.render(BEAM, SIGMA_S, SIGMA_A, G, RES, paths=PATHS, batches=K, seed=4, max_depth=2)
    column_check(sums, SIGMA_S + SIGMA_A, PATHS, "ballistic column")


def test_box_that_cuts_the_shape():
    """a 4 x 6 x 5 grid over a box that cuts the cube: deposits outside it go to `dropped`, and the balance counts them"""
    sums, tot = F.render(BEAM, SIGMA_S, SIGMA_A, G, paths=PATHS, batches=K, seed=5, **CUT)
    assert sums.shape == (K, 5, 6, 4) and np.all(tot[:, 4] > 0)
    bal = SIGMA_A * (sums.sum((1, 2, 3)) + tot[:, 4]) + tot[:, 1]
    F.total_bar(bal, PATHS * POWER, what="cut balance")
    # first collisions: the part of the column inside the box (x = 0.2 -> cell 3 of 4, y = 0.1 -> cell 2 of 6, z up to 0.25)
    s1, t1 = F.render(BEAM, 0.0, ABSORBER, 0.0, paths=PATHS, batches=K, seed=6, **CUT)
    column_check(s1, ABSORBER, PATHS, "cut column", **CUT)
    assert np.all(s1[:, :, 2, 3] > 0) and np.all(t1[:, 4] > 0)
    np.testing.assert_allclose(ABSORBER * (s1.sum((1, 2, 3)) + t1[:, 4]) + t1[:, 1], PATHS * POWER, rtol=1e-12)


def test_point_emitter_inside_balances():
    em = F.point([0.05, -0.04, 0.02], 2.0)
    sums, tot = F.render(em, SIGMA_S, SIGMA_A, G, RES, paths=PATHS, batches=K, seed=7)
    bal = SIGMA_A * sums.sum((1, 2, 3)) + tot[:, 1]
    F.total_bar(bal, PATHS * em["phi"], what="point balance")
    # roulette on from the first scattering: the same expectation
    s2, t2 = F.render(em, SIGMA_S, SIGMA_A, G, RES, paths=PATHS, batches=K, seed=8, rr_depth=1)
    F.total_bar(SIGMA_A * s2.sum((1, 2, 3)) + t2[:, 1], PATHS * em["phi"], what="point balance, rr_depth 1")
    F.bar(sums.mean(0), sums.std(0, ddof=1) / np.sqrt(K), s2.mean(0), s2.var(0, ddof=1) / K, what="rr_depth 5 vs 1")
