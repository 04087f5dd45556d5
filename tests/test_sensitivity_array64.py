"""tests/sensitivity_array64.py, the float64 restatement of the sensitivity grids of an array of detectors and gates
(mer_sensitivity_array_create), against tests/sensitivity64.py, whose walk it copies, and against the derivative of the detected signal
by sigma_s.  No GPU.  The module also holds the reference of tests/test_gpu_sensitivity_array.py and its checks.

Set-up: test_sensitivity64's: the cube [-1, 1]^3, the beam of power (5, 3, 8) from (0.25, 0.25, -3) along +z, 4^3 cells, a 4 x 4 raster on
face 5."""
import functools
import numpy as np
from tests import sensitivity64 as S
from tests import sensitivity_array64 as A
from tests import test_sensitivity64 as T

SCATTER = dict(sigma_s=np.array([1.0, 0.8, 1.3]), sigma_a=np.array([0.2, 0.3, 0.1]), g=0.5)      # test_gpu_sensitivity.SCATTER's medium
RAGGED = T.RAGGED


def _medium():
    return S.LP.homogeneous(SCATTER["sigma_s"], SCATTER["sigma_a"], "balance")


def test_one_bin_one_gate_is_sensitivity64():
    """the copy is pinned: one detector, one gate, the same seed -- the same draws in the same order -- give sensitivity64.render's J and
    totals, with a cone and a gate and into a ragged box"""
    kw = dict(paths=2048, batches=2, seed=13, bmin=RAGGED["bmin"], bmax=RAGGED["bmax"])
    gate = dict(cos_min=0.3, t_min=2.0, t_bin=3.5)
    ref, rt = S.render(T.BEAM, T.POWER3, _medium(), SCATTER["g"], RAGGED["res"], S.detector((4, 4), 5, (1, 4, 0, 3), **gate), **kw)
    j, k, meas, t = A.render(T.BEAM, T.POWER3, _medium(), SCATTER["g"], RAGGED["res"], A.array((4, 4), 5, (1, 4, 0, 3), **gate), **kw)
    assert j.shape == (2, 1, 1, 1, 3, 4, 5, 3) and rt[:, 8].min() > 64
    np.testing.assert_allclose(j[:, 0, 0, 0], ref, rtol=1e-12, atol=0)
    np.testing.assert_allclose(t[:, :13], rt[:, :13], rtol=1e-12, atol=0)
    np.testing.assert_allclose(meas[:, 0, 0, 0, :3], rt[:, 1:4], rtol=1e-12, atol=0)
    assert np.array_equal(meas[:, 0, 0, 0, 3], rt[:, 8])
    # the collisions: cells + outside the box = all of them, per channel
    assert np.all(t[:, 13:16] > 0) and k.sum() > 0
    np.testing.assert_allclose(k.reshape(2, -1, 3).sum(1) + t[:, 13:16], meas[:, 0, 0, 0, 4:7], rtol=1e-12, atol=0)


def test_measurements_partition_the_whole_window():
    """J summed over the 2 x 2 detectors and the 4 gates of [4, 6) is the J of the one detector with the whole window and the one gate
    [4, 6); so are K and the measurements.  Every gate and every detector takes some paths"""
    kw = dict(paths=4096, batches=1, seed=17)
    j1, k1, m1, t1 = A.render(T.BEAM, T.POWER3, _medium(), SCATTER["g"], T.RES, A.array((4, 4), 5, T.WHOLE, t_min=4.0, t_bin=2.0), **kw)
    j, k, m, t = A.render(T.BEAM, T.POWER3, _medium(), SCATTER["g"], T.RES, A.array((4, 4), 5, T.WHOLE, bins=(2, 2), gates=4, t_min=4.0, t_bin=0.5), **kw)
    assert j.shape == (1, 4, 2, 2, 4, 4, 4, 3) and np.all(m[0, ..., 3].sum((1, 2)) > 0) and np.all(m[0, ..., 3].sum(0) > 0)
    np.testing.assert_allclose(j.sum((1, 2, 3)), j1[:, 0, 0, 0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(k.sum((1, 2, 3)), k1[:, 0, 0, 0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(m.sum((1, 2, 3)), m1[:, 0, 0, 0], rtol=1e-12, atol=0)
    np.testing.assert_allclose(t, t1, rtol=1e-12, atol=0)
    np.testing.assert_allclose(m[..., :4].sum((1, 2, 3)), t[:, [1, 2, 3, 8]], rtol=1e-12, atol=0)


def deriv_array(sigma_s_shift, seed=5, paths=2 * T.PATHS, bins=(1, 1), gates=1, t_min=0.0, t_bin=0.0):
    D = T.DERIV
    m = S.manual(D["sigma_s"] + sigma_s_shift, D["sigma_a"], D["density"], D["weight"])
    det = A.array((4, 4), 5, D["det"]["window"], bins=bins, gates=gates, cos_min=D["det"]["cos_min"], t_min=t_min, t_bin=t_bin)
    return A.render(T.BEAM, T.POWER3, m, D["g"], T.RES, det, paths=paths, batches=1, seed=seed, rr_depth=D["rr_depth"], max_depth=D["max_depth"])


def test_scattering_jacobian_is_the_derivative_of_the_signal():
    """strategy manual at a fixed density, no roulette, at most 20 flights: the walks at sigma_s +- delta draw the same paths, and a detected
    path's weight is w = (a factor free of sigma_s) x sigma_s^N exp(-sigma_s L) per channel, N its scattering collisions and L its length:
    dw / dsigma_s = w (N / sigma_s - L), so the derivative of the detected weight of measurement m is sum(K[m]) / sigma_s - sum(J[m]).
    The central difference of w over +- delta is w (N / sigma_s - L) (1 + O(delta^2 (N / sigma_s - L)^2)): with at most 20 flights of at
    most 2 sqrt(3), L < 70 and N <= 20, N / sigma_s <= 20 / 0.9 < 23, so |N / sigma_s - L| < 70 and the relative truncation is at most
    delta^2 70^2 / 6 = 8.2e-4 per path as in the sigma_a test -- but of terms of either sign: the two sums cancel, so the tolerance is
    DERIV_RTOL times sum(K) / sigma_s + sum(J), the sum of the magnitudes, not times their difference.  Per measurement of a 2 x 2 array."""
    D = T.DERIV
    d = D["delta"]
    j, k, m, t = deriv_array(0.0)
    _, _, mp, tp = deriv_array(+d)
    _, _, mm, tm = deriv_array(-d)
    assert np.array_equal(mp[..., 3], mm[..., 3]) and np.array_equal(mp[..., 3], m[..., 3])             # the same paths
    assert m.shape == (1, 1, 2, 2, 8) and np.all(m[..., 3] > 64)
    diff = (mp[0, ..., :3] - mm[0, ..., :3]) / (2 * d)                      # (1, 2, 2, 3)
    ks, js = k[0].sum((3, 4, 5)) / D["sigma_s"], j[0].sum((3, 4, 5))
    print("dW/dsigma_s", diff.reshape(-1, 3), "sum(K)/sigma_s - sum(J)", (ks - js).reshape(-1, 3), "error / tolerance", (np.abs(diff - (ks - js)) / (T.DERIV_RTOL * (ks + js))).max())
    assert np.all(np.abs(diff - (ks - js)) <= T.DERIV_RTOL * (ks + js))
    # the box is the cube: every collision has a cell
    assert not t[0, 13:16].any()
    np.testing.assert_allclose(k[0].sum((3, 4, 5)), m[0, ..., 4:7], rtol=1e-12, atol=0)


# ---- the reference of tests/test_gpu_sensitivity_array.py ----------------------------------------------------------------------------------
# 16 batches of 16 384 paths, 4^3 cells, face 5, the whole window in 2 x 2 bins, two gates of width 1 from 4 on, the scattering grids too

K_BATCHES = 16
REF_PATHS = 16384
REF_ARRAY = dict(bins=(2, 2), gates=2, t_min=4.0, t_bin=1.0)


@functools.lru_cache(maxsize=None)
def array_ref(which=0):
    """(J, K, meas, totals) of the case, computed once; which = 0: the reference the GPU is held to, 1: another seed"""
    return A.render(T.BEAM, T.POWER3, _medium(), SCATTER["g"], T.RES, A.array((4, 4), 5, T.WHOLE, **REF_ARRAY), paths=REF_PATHS, batches=K_BATCHES,
                    seed=521 + 7 * which)


def compared_grids(j, k):
    """the grids the issue compares per cell: J and K of each of the four gate-0 measurements, and of gate 1 summed over its detectors:
    {name: (batches, nz, ny, nx, 3)}"""
    out = {}
    for name, g in (("J", j), ("K", k)):
        for dv in range(2):
            for du in range(2):
                out["%s gate 0 detector (%d, %d)" % (name, du, dv)] = g[:, 0, dv, du]
        out["%s gate 1, all detectors" % name] = g[:, 1].sum((1, 2))
    return out


def check_array(got, ref, what):
    """got, ref = (J, K, meas, totals) in batches: every compared grid cell by cell under the bar (cells the reference leaves empty in all
    batches are not compared singly; at most a quarter of a grid's cells), its 12 slab sums, every meas entry and every total within
    4 sigma.  Returns (largest cell z, cells beyond 4 sigma, largest slab z, largest meas z, largest total z, fewest compared cells)"""
    k = len(ref[0])
    zc, beyond, zs, fewest = 0.0, 0, 0.0, 64
    gg, rg = compared_grids(got[0], got[1]), compared_grids(ref[0], ref[1])
    for name in rg:
        a, r = gg[name], rg[name]
        on = r.max(0) > 0
        on_cells = on.any(-1)
        assert 4 * on_cells.sum() >= 3 * on_cells.size, (what, name, "the reference leaves more than a quarter of the cells empty", int(on_cells.sum()))
        fewest = min(fewest, int(on_cells.sum()))
        z = S.bar(a[:, on].mean(0), a[:, on].std(0, ddof=1) / np.sqrt(len(a)), r[:, on].mean(0), r[:, on].var(0, ddof=1) / k, what="%s %s cells" % (what, name))
        zc, beyond = max(zc, float(z.max())), beyond + int((z > 4).sum())
        sa, sr = T.slabs(a), T.slabs(r)
        for ax in range(3):
            for i in range(sa.shape[2]):
                for c in range(3):
                    if sr[:, ax, i, c].var() > 0:
                        zs = max(zs, S.total_bar(sa[:, ax, i, c], sr[:, ax, i, c].mean(), sr[:, ax, i, c].var(ddof=1) / k, what="%s %s slab %s %d channel %d" % (what, name, "xyz"[ax], i, c)))
    m, rm = got[2].reshape(len(got[2]), -1), ref[2].reshape(k, -1)
    zm = max(S.total_bar(m[:, q], rm[:, q].mean(), rm[:, q].var(ddof=1) / k, what="%s meas[%d][%d]" % (what, q // 8, q % 8)) for q in range(m.shape[1]) if q % 8 != 7)
    assert not m[:, 7::8].any()
    t, rt = got[3], ref[3]
    assert np.all(t[:, 0] == rt[:, 0]) and not t[:, 7].any() and not t[:, 12].any() and not t[:, 4:7].any() and not t[:, 13:16].any()
    zt = max(S.total_bar(t[:, q], rt[:, q].mean(), rt[:, q].var(ddof=1) / k, what="%s totals[%d]" % (what, q)) for q in (1, 2, 3, 8, 9, 10, 11))
    return zc, beyond, zs, float(zm), float(zt), fewest


def test_the_gpu_case_passes_reference_against_reference():
    """the condition under which the case may hold the GPU: two seeds of the restatement against each other pass every check the GPU is
    put to, the cap on the cells left out included (both seeds as the reference)"""
    a, b = array_ref(1), array_ref(0)
    print("detected paths per batch, gate x dv x du:", b[2][..., 3].mean(0).reshape(2, -1))
    print("seed 1 against seed 0 (cell z, beyond, slab z, meas z, total z, fewest compared cells):", check_array(a, b, "seed against seed"))
    print("seed 0 against seed 1:", check_array(b, a, "seed against seed, swapped"))
