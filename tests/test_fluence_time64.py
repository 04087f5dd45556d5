"""tests/fluence_time64.py, the float64 restatement of the time-resolved fluence estimator (include/mer.h, mer_fluence_time_create), pinned
by what such a grid must obey whatever the code: along an unscattered beam the deposits of frame f are Beer-Lambert over the depths the
pulse crosses during that frame, with the index n stretching the path length inside the medium and the exterior leg counted at index 1;
exact zeros off the beam and in frames the pulse cannot reach; the weight that falls outside the window is accounted for.
tests/test_gpu_fluence_time.py holds the GPU against the same closed form and against this restatement.  No GPU, no library.

Set-up shared with the GPU tests (tests/test_fluence64.py): the cube [-1, 1]^3, the beam of power 5 from (0.2, 0.1, -3) along +z (an
exterior leg of 2), K = 16 batches of 16 384 paths.

The absorber case: an 8 x 8 x 8 grid, 8 frames from t_min = 1.9 of width 0.35.  With n = 1.4 the frame edges fall at the depths
-0.0714 + 0.25 f: every z cell is split between two frames, and the window ends at the depth z* = 2.7 / 1.4 = 1.9286 in front of the exit
face, so 0.56 % of the paths deposit outside it.  With n = 1 the edges fall at -0.1 + 0.35 f, the window holds every deposit and frames
6 and 7 stay empty.

The scattering case: a 4 x 4 x 4 grid, 6 frames from t_min = 2 of width 1, seeds SC_SEEDS: two runs of the restatement satisfy the
project's bar against each other at this size (no coarsening was needed), which is what entitles the GPU test to hold the kernel to it."""
import functools
import numpy as np
import pytest
from tests import fluence_time64 as FT
from tests import test_fluence64 as T

ABS = dict(res=(8, 8, 8), frames=8, t_min=1.9, t_bin=0.35)
RIF_CONSTS = (1.4, 1.0)
SC = dict(res=(4, 4, 4), frames=6, t_min=2.0, t_bin=1.0)
SC_SEEDS = (21, 22)
PATHS, K = T.PATHS, T.K


def column_time_check(sums, tot8, sigma_t, rif_const, paths, what):
    """(batches, frames, nz, ny, nx) raw sums of FIRST collisions of the beam and (batches,) out-of-window weights against the closed form:
    every (frame, cell) of the column within the bar under the binomial variance, every bin off the column and every bin of a frame the
    closed form excludes exactly 0, the absorbed power outside the window sigma_t totals[8] against paths P p_late"""
    p, p_late = FT.beam_column_time(T.BEAM, sigma_t, rif_const, **ABS)
    k = len(sums)
    ref = paths * T.POWER / sigma_t * p
    sd = np.sqrt(paths * (T.POWER / sigma_t) ** 2 * p * (1 - p) / k)
    on = p > 0
    assert on.any()
    assert np.all(sums[:, ~on] == 0.0), "deposits off the beam's column or in a frame the pulse cannot reach"
    FT.bar(sums.mean(0)[on], sd[on], ref[on], what=what)
    if p_late > 1e-12:
        FT.total_bar(sigma_t * tot8, paths * T.POWER * p_late, what=what + ", out of window")
    else:
        assert np.all(tot8 == 0.0)
    return p, p_late


@pytest.mark.parametrize("rif_const", RIF_CONSTS)
def test_pure_absorber_is_beer_lambert_per_frame(rif_const):
    sums, tot = FT.render(T.BEAM, 0.0, T.ABSORBER, 0.0, rif_const=rif_const, paths=PATHS, batches=K, seed=31, **ABS)
    p, p_late = column_time_check(sums, tot[:, 8], T.ABSORBER, rif_const, PATHS, "absorber column, n = %g" % rif_const)
    if rif_const == 1.4:
        zs = (ABS["t_min"] + ABS["frames"] * ABS["t_bin"] - 2.0) / 1.4
        np.testing.assert_allclose(p_late, np.exp(-T.ABSORBER * zs) - np.exp(-2 * T.ABSORBER), rtol=1e-12)
        assert 0.005 < p_late < 0.006 and np.all(tot[:, 8] > 0)
        assert np.all(p.sum((1, 2, 3)) > 0)                             # the pulse crosses the cube during all 8 frames
        assert np.all((p > 0).sum((0, 2, 3)) == [2] * 7 + [1])          # every z cell of the column is split: between two frames, the last between frame 7 and the time after the window
    else:
        assert p_late < 1e-12 and not p[6:].any() and p[5].any()       # the pulse has left after frame 5
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:8] == 0) and np.all(tot[:, 11] == 0)
    # every path deposits P / sigma once, inside or outside the window, or escapes with P
    np.testing.assert_allclose(T.ABSORBER * (sums.sum((1, 2, 3, 4)) + tot[:, 8]) + tot[:, 1], PATHS * T.POWER, rtol=1e-12)


@functools.lru_cache(maxsize=None)
def scattering_ref(seed):
    """the float64 reference of the scattering case, computed once per seed"""
    return FT.render(T.BEAM, T.SIGMA_S, T.SIGMA_A, T.G, paths=PATHS, batches=K, seed=seed, rr_depth=5, **SC)


def against(sums, tot, ref, what):
    """(K, frames, nz, ny, nx) sums and (K, 12) totals against a reference run: per bin within the bar with both batch spreads, the
    escaped, dropped and out-of-window totals within 4 sigma"""
    r, rt = ref
    FT.bar(sums.mean(0), sums.std(0, ddof=1) / np.sqrt(K), r.mean(0), r.var(0, ddof=1) / K, what=what + " bins")
    for q, name in ((1, "escaped"), (4, "dropped"), (8, "out of window")):
        if rt[:, q].any():
            FT.total_bar(tot[:, q], rt[:, q].mean(), rt[:, q].var(ddof=1) / K, what="%s %s" % (what, name))
        else:
            assert not tot[:, q].any(), name


def test_scattering_restatement_satisfies_the_bar_against_itself():
    a, ta = scattering_ref(SC_SEEDS[0])
    b, tb = scattering_ref(SC_SEEDS[1])
    against(b, tb, (a, ta), "self")
    assert np.all(ta[:, 8] > 0) and (a.mean(0)[-1] > 0).all()          # some light arrives after the window, and the last frame reaches every cell
    # the window takes nothing away: in and out of it, absorbed plus escaped is what was emitted
    bal = T.SIGMA_A * (a.sum((1, 2, 3, 4)) + ta[:, 8]) + ta[:, 1]
    FT.total_bar(bal, PATHS * T.POWER, what="balance")


def test_sum_over_a_window_that_holds_everything_is_the_steady_state_grid():
    """the same seed: the timed restatement draws what tests/fluence64.py draws, so the frames add up to its grid"""
    from tests import fluence64 as F
    s, t = F.render(T.BEAM, T.SIGMA_S, T.SIGMA_A, T.G, (4, 4, 4), paths=4096, batches=2, seed=5, max_depth=6)
    st, tt = FT.render(T.BEAM, T.SIGMA_S, T.SIGMA_A, T.G, (4, 4, 4), 32, 0.0, 1.0, paths=4096, batches=2, seed=5, max_depth=6)
    assert not tt[:, 8:].any()
    np.testing.assert_allclose(st.sum(1), s, rtol=1e-12, atol=0)
    np.testing.assert_array_equal(tt[:, :8], t)
