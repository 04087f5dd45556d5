"""tests/fluence_track64.py, the float64 restatement of the track-length fluence estimator (include/mer.h, mer_fluence_track_create), pinned
by closed forms and by the collision estimator's restatement (tests/fluence64.py): both estimate the same fluence.
tests/test_gpu_fluence_track.py holds the GPU against the same closed forms and against this restatement.  No GPU, no library.

The set-up is tests/test_fluence64.py's: the cube [-1, 1]^3, the beam of power 5 from (0.2, 0.1, -3) along +z, an 8^3 grid, K = 16 batches
of 16 384 paths.  The bar is the project's (fluence64.bar / total_bar)."""
import functools
import numpy as np
from tests import fluence64 as F
from tests import fluence_track64 as FT
from tests import test_fluence64 as T

POWER, BEAM, RES, PATHS, K = T.POWER, T.BEAM, T.RES, T.PATHS, T.K
CHROMATIC = (1.0, 1.5, 2.0)                    # sigma_a per channel; strategy single samples the smallest: rho = 1.0
RAMP_MAX = 4.0                                 # sigma_t(z) = RAMP_MAX (z + 1) / 2


def ramp_sigma(p):
    return RAMP_MAX * (p[:, 2] + 1) / 2


def absorber_column_check(sums, sigma, paths, what, res=RES, bmin=(-1, -1, -1), bmax=(1, 1, 1)):
    """(batches, nz, ny, nx) raw sums of the analog pure absorber: the column within the bar under the closed-form variance, every other cell
    exactly 0.0; returns batch sd / closed-form sd over the column"""
    on, a, b = FT.column_depths(BEAM, res, bmin, bmax)
    assert on.any()
    assert np.all(sums[:, ~on] == 0.0), "deposits off the beam's column"
    k = len(sums)
    mean, second = FT.absorber_moments(POWER, sigma, a, b)
    mean = np.broadcast_to(mean[:, None, None], on.shape)[on]; second = np.broadcast_to(second[:, None, None], on.shape)[on]
    sd = np.sqrt(paths * (second - mean ** 2) / k)
    F.bar(sums.mean(0)[on], sd, paths * mean, what=what)
    return sums[:, on].std(0, ddof=1) / np.sqrt(k) / sd


def mean_column_check(sums, ref_per_path, paths, what, res=RES, bmin=(-1, -1, -1), bmax=(1, 1, 1)):
    """the column against a closed-form mean (ref_per_path(a, b) per slab) under the batch spread; every other cell exactly 0.0"""
    on, a, b = FT.column_depths(BEAM, res, bmin, bmax)
    assert np.all(sums[:, ~on] == 0.0), "deposits off the beam's column"
    ref = np.broadcast_to((paths * ref_per_path(a, b))[:, None, None], on.shape)[on]
    return F.bar(sums.mean(0)[on], sums[:, on].std(0, ddof=1) / np.sqrt(len(sums)), ref, what=what)


@functools.lru_cache(maxsize=None)
def scattering(seed=2):
    return FT.render(BEAM, T.SIGMA_S, T.SIGMA_A, T.G, RES, paths=PATHS, batches=K, seed=seed)


def test_pure_absorber_column_has_the_closed_form_mean_and_variance():
    sums, tot = FT.render(BEAM, 0.0, T.ABSORBER, 0.0, RES, paths=PATHS, batches=K, seed=1)
    ratio = absorber_column_check(sums, T.ABSORBER, PATHS, "track absorber column")
    print("batch sd / closed-form sd: %.2f ... %.2f" % (ratio.min(), ratio.max()))
    assert 0.3 < ratio.min() and ratio.max() < 1.9      # sqrt(chi^2_15 / 15): mean 1, sd 1 / sqrt(30) = 0.18: within 4 sigma and a little
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:] == 0)
    F.total_bar(tot[:, 1], PATHS * POWER * np.exp(-2 * T.ABSORBER), what="track absorber escaped")
    # the balance holds in expectation, not per path
    F.total_bar(T.ABSORBER * sums.sum((1, 2, 3)) + tot[:, 1], PATHS * POWER, what="track absorber balance")


def test_max_depth_2_keeps_the_first_flights():
    sums, tot = FT.render(BEAM, T.SIGMA_S, T.SIGMA_A, T.G, RES, paths=PATHS, batches=K, seed=4, max_depth=2)
    absorber_column_check(sums, T.SIGMA_S + T.SIGMA_A, PATHS, "track ballistic column")


def test_scattering_medium_agrees_with_the_collision_estimator():
    sums, tot = scattering()
    ref, rt = F.render(BEAM, T.SIGMA_S, T.SIGMA_A, T.G, RES, paths=PATHS, batches=K, seed=3)
    F.bar(sums.mean(0), sums.std(0, ddof=1) / np.sqrt(K), ref.mean(0), ref.var(0, ddof=1) / K, what="track vs collision")
    F.total_bar(tot[:, 1], rt[:, 1].mean(), rt[:, 1].var(ddof=1) / K, what="track vs collision escaped")
    assert np.all(tot[:, 4:] == 0)
    F.total_bar(T.SIGMA_A * sums.sum((1, 2, 3)) + tot[:, 1], PATHS * POWER, what="track balance")
    assert (sums > 0).all()                                                # every cell is crossed in every batch
    # equal paths, less noise: the median per-cell variance ratio collision / track
    ratio = np.median(ref.var(0, ddof=1) / sums.var(0, ddof=1))
    print("median variance ratio collision / track: %.2f" % ratio)
    assert ratio > 1


def test_box_that_cuts_the_shape():
    """weight x length outside the box goes to `dropped`, and the balance counts it"""
    sums, tot = FT.render(BEAM, T.SIGMA_S, T.SIGMA_A, T.G, paths=PATHS, batches=K, seed=5, **T.CUT)
    assert sums.shape == (K, 5, 6, 4) and np.all(tot[:, 4] > 0)
    F.total_bar(T.SIGMA_A * (sums.sum((1, 2, 3)) + tot[:, 4]) + tot[:, 1], PATHS * POWER, what="track cut balance")
    ref, rt = F.render(BEAM, T.SIGMA_S, T.SIGMA_A, T.G, paths=PATHS, batches=K, seed=6, **T.CUT)
    F.bar(sums.mean(0), sums.std(0, ddof=1) / np.sqrt(K), ref.mean(0), ref.var(0, ddof=1) / K, what="track vs collision, cut")
    F.total_bar(tot[:, 4], rt[:, 4].mean(), rt[:, 4].var(ddof=1) / K, what="track vs collision, cut dropped")
    s1, t1 = FT.render(BEAM, 0.0, T.ABSORBER, 0.0, paths=PATHS, batches=K, seed=7, **T.CUT)
    absorber_column_check(s1, T.ABSORBER, PATHS, "track cut column", **T.CUT)
    assert np.all(s1[:, :, 2, 3] > 0) and np.all(t1[:, 4] > 0)


def test_chromatic_absorber_with_one_sampling_channel():
    """sigma_a = (1, 1.5, 2) sampled with rho = 1 (strategy single): channel c holds P (e^{-sigma_c a} - e^{-sigma_c b}) / sigma_c"""
    sums, tot = FT.render(BEAM, 0.0, CHROMATIC, 0.0, RES, paths=PATHS, batches=K, seed=8, rho=min(CHROMATIC))
    assert sums.shape == (K, 8, 8, 8, 3)
    for c, s in enumerate(CHROMATIC):
        mean_column_check(sums[..., c], lambda a, b: FT.beer_mean(POWER, s, a, b), PATHS, "track chromatic column, channel %d" % c)
    # the smaller sigma_t, the more light in every column cell
    on, a, b = FT.column_depths(BEAM, RES)
    assert np.all(sums[..., 0][:, on] > sums[..., 2][:, on])


def test_sigma_ramp_with_delta_tracking():
    """sigma_t(z) = 4 (z + 1) / 2, albedo 0: the column against P sqrt(pi) / 2 (erf(b') - erf(a')), escaped fraction e^{-4}"""
    sums, tot = FT.render(BEAM, None, None, 0.0, RES, paths=PATHS, batches=K, seed=9, sigma_fn=ramp_sigma, sigma_max=RAMP_MAX, albedo=0.0)
    mean_column_check(sums, lambda a, b: FT.ramp_mean(POWER, 1.0, a, b), PATHS, "track ramp column")
    F.total_bar(tot[:, 1], PATHS * POWER * np.exp(-4.0), what="track ramp escaped")
    # the entry cell, where sigma_t starts at 0: the relative standard error stays small (the collision estimator's 1 / sigma blows up there)
    on, a, b = FT.column_depths(BEAM, RES)
    col = sums[:, on]
    rel = col[:, 0].std(ddof=1) / np.sqrt(K) / col[:, 0].mean()
    print("entry cell: relative standard error %.1e" % rel)
    assert rel < 2e-3        # a path deposits P min(t, 0.25) there and 94 % cross the whole cell: relative sd per path below 0.25, / sqrt(K PATHS) = 5e-4
