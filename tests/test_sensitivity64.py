"""tests/sensitivity64.py, the float64 restatement of the sensitivity grid (mer_render_sensitivity), against three closed forms and, for
the sigma_t ramp, against a closed form and tests/lightpath64.py's exitance map and track-length grid.  No GPU.  The module also holds the
cases, the cached references and the checks of tests/test_gpu_sensitivity_media.py.

Set-up: the cube [-1, 1]^3, the beam of power (5, 3, 8) from (0.25, 0.25, -3) along +z, grids of 4^3 cells over the cube, the detector a
window of a 4 x 4 raster on face 5 (z = +1).  The beam meets raster cell (iu, iv) = (2, 2) and grid column ix = iy = 2."""
import functools
import numpy as np
import pytest
from tests import sensitivity64 as S
from tests import test_lightpath64 as L

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


# ---- the sigma_t ramp, any face --------------------------------------------------------------------------------------------------------------
# (tests/test_lightpath64.py's media and beam: the ramp 0.5 ... 4 along z with the albedo (0.9, 0.6, 0.3), the beam from (0.2, 0.1, -3))

K = L.K
WHOLE = (0, 4, 0, 4)
POINT_O = (0.1, -0.2, 0.3)
POINT_I = (1.0, 0.8, 0.5)                               # the point emitter's intensity; 4 pi I per path
POINT_POWER = 4.0 * np.pi * np.array(POINT_I)
RAGGED = dict(res=(5, 4, 3), bmin=(-0.6, -0.5, -0.7), bmax=(0.5, 0.7, 0.4))       # a box that cuts the cube, no face at a round number
NO_RR = 100000


def test_absorbing_ramp_column():
    """albedo 0: a path is detected iff its first flight passes the cube, with w = P exactly (no strategy factor in a ramp): J_c = detected
    P 2 / nz on the beam's column given the count, exactly 0 elsewhere; the count is binomial with p = exp(-4.5), the optical depth of the
    column.  Observed: 346 detected of 32 768, expected 364.0, z 0.95"""
    k = 8
    m = S.LP.ramp(L.RAMP["s_lo"], L.RAMP["s_hi"], 0.0)
    j, t = S.render(BEAM, POWER3, m, 0.0, RES, BEAM_CELL, paths=PATHS, batches=k, seed=3)
    on = column(j)
    assert np.all(j[:, ~on] == 0.0)
    for b in range(k):
        np.testing.assert_allclose(j[b][on], np.broadcast_to(t[b, 8] * POWER3 * 0.5, (4, 3)), rtol=1e-12, atol=0)
        np.testing.assert_allclose(t[b, 1:4], t[b, 8] * POWER3, rtol=1e-12, atol=0)
    assert abs(S.LP.ramp_depth(m, 2.0) - 4.5) < 1e-12
    p = np.exp(-S.LP.ramp_depth(m, 2.0))
    z = abs(t[:, 8].sum() - k * PATHS * p) / np.sqrt(k * PATHS * p * (1 - p))
    print("detected %d of %d, expected %.1f, z %.2f" % (t[:, 8].sum(), k * PATHS, k * PATHS * p, z))
    assert z <= 4 and t[:, 8].sum() > 0


@functools.lru_cache(maxsize=None)
def _ramp_tmap():
    return S.LP.render(L.beam(), L.POWER3, S.LP.ramp(**L.RAMP), L.G, emap=L.TMAP, paths=PATHS, batches=K, seed=71)


@pytest.mark.parametrize("face", range(6))
def test_ramp_detected_weight_is_the_exitance_window(face):
    """the scattering ramp: the detected weight of a whole-face detector under the cone (cos_min 0.3) and the gate [2, 5) of path length
    against lightpath64's timed map TMAP of the same cone, whose three frames of width 1 from 2 on are summed; independent seeds, per
    channel within 4 sigma.  The grid is one cell: the detector does not depend on it.  Observed: z <= 2.25 over the 18 totals"""
    det = S.detector((4, 4), face, WHOLE, cos_min=L.TMAP["cos_min"], t_min=L.TMAP["t_min"], t_bin=L.TMAP["frames"] * L.TMAP["t_bin"])
    _, t = S.render(L.beam(), L.POWER3, S.LP.ramp(**L.RAMP), L.G, (1, 1, 1), det, paths=PATHS, batches=K, seed=80 + face)
    m = _ramp_tmap()["emap"][:, :, face].sum((1, 2, 3))                  # (K, 3): frames and cells summed
    assert np.all(t[:, 8] > 0) and np.all(t[:, 12] == 0)
    for c in range(3):
        S.total_bar(t[:, 1 + c], m[:, c].mean(), m[:, c].var(ddof=1) / K, what="ramp face %d channel %d detected weight against the map" % (face, c))


def test_six_faces_sum_to_the_track_grid():
    """the float64 twin of "every path is detected": the ramp with albedo 1, the roulette out of reach.  Every path leaves through exactly
    one face with w = P, so the six whole-face detectors, rendered with one seed (the detector draws no number: the same paths), sum to
    w^T L over all paths -- the track-length grid of lightpath64 (T P l per piece), rendered with another seed.  Cells within the bar,
    dropped and weight x length within 4 sigma.  Observed: 0 of 180 cells beyond 4 sigma, max z 3.80; totals z <= 0.20"""
    k, paths = 8, 2048
    med = S.LP.ramp(L.RAMP["s_lo"], L.RAMP["s_hi"], (1.0, 1.0, 1.0))
    kw = dict(paths=paths, batches=k, rr_depth=NO_RR)
    js, ts = zip(*[S.render(L.beam(), L.POWER3, med, L.G, RAGGED["res"], S.detector((4, 4), f, WHOLE), bmin=RAGGED["bmin"], bmax=RAGGED["bmax"],
                            seed=90, **kw) for f in range(6)])
    j, t = sum(js), sum(ts)
    assert np.all(t[:, 8] == paths) and min(x[:, 8].sum() for x in ts) > 0          # no exit belongs to two faces or to none
    np.testing.assert_allclose(t[:, 1:4], np.broadcast_to(paths * np.array(L.POWER3), (k, 3)), rtol=1e-12, atol=0)
    np.testing.assert_allclose(j.reshape(k, -1, 3).sum(1) + t[:, 4:7], t[:, 9:12], rtol=1e-9, atol=0)
    ref = S.LP.render(L.beam(), L.POWER3, med, L.G, track=RAGGED, seed=91, **kw)
    r, rt = ref["track"], ref["track_totals"]
    assert (r.mean(0) > 0).all()
    S.bar(j.mean(0), j.std(0, ddof=1) / np.sqrt(k), r.mean(0), r.var(0, ddof=1) / k, what="six faces against the track grid")
    rin = r.reshape(k, -1, 3).sum(1) + rt[:, 4:7]
    for c in range(3):
        S.total_bar(t[:, 4 + c], rt[:, 4 + c].mean(), rt[:, 4 + c].var(ddof=1) / k, what="dropped, channel %d" % c)
        S.total_bar(t[:, 9 + c], rin[:, c].mean(), rin[:, c].var(ddof=1) / k, what="weight x length, channel %d" % c)


# ---- the references of tests/test_gpu_sensitivity_media.py -------------------------------------------------------------------------------------
# K = 16 batches of 16 384 paths, a 4^3 grid over the cube, a 4 x 4 raster.  medium / emitter / detector / n; the GPU file builds the same scenes.

CONE_GATE = dict(cos_min=0.3, t_min=0.5, t_bin=3.0)
CASES = {
    "ramp, forward": dict(medium=("ramp", None), emitter="beam", face=5),
    "ramp, back-scatter": dict(medium=("ramp", None), emitter="beam", face=4),
    "ramp, side, cone and gate": dict(medium=("ramp", None), emitter="point", face=0, **CONE_GATE),
    "ramp with albedo grid": dict(medium=("ramp", "grid"), emitter="point", face=4),
    "maximum, weight 0.7, n = 1.33": dict(medium=("maximum", "strong", 0.7), emitter="point", face=5, n=1.33, **CONE_GATE),
    "single, weight 0.7": dict(medium=("single", "mild", 0.7), emitter="point", face=5),
}
CASE_SEEDS = {name: 300 + 20 * i for i, name in enumerate(CASES)}             # seed of the reference `which`: this + 5 which
CASE_PATHS = L.PATHS


def case_medium(name):
    m = CASES[name]["medium"]
    if m[0] == "ramp":
        from tests import scenes
        return S.LP.ramp(L.RAMP["s_lo"], L.RAMP["s_hi"], L.RAMP["albedo"] if m[1] is None else scenes.rgb_albedo(8).astype(np.float64))
    return S.LP.homogeneous(strategy=m[0], weight=m[2], **L.CHROMA[m[1]])


@functools.lru_cache(maxsize=None)
def case_ref(name, which=0):
    """(J (K, 4, 4, 4, 3), totals (K, 16)) of the case from tests/sensitivity64.py, computed once; which = 0: the reference the GPU is held to,
    1, 2, ...: further seeds"""
    c = CASES[name]
    beam = c["emitter"] == "beam"
    det = S.detector((4, 4), c["face"], WHOLE, cos_min=c.get("cos_min", 0.0), t_min=c.get("t_min", 0.0), t_bin=c.get("t_bin", 0.0))
    return S.render(L.beam() if beam else S.point(POINT_O, 1.0), L.POWER3 if beam else POINT_POWER, case_medium(name), L.G, RES, det,
                    n=c.get("n", 1.0), paths=CASE_PATHS, batches=K, seed=CASE_SEEDS[name] + 5 * which)


def slabs(j):
    """the three slab profiles of J (K, nz, ny, nx, 3): J summed over each plane normal to x, y and z: (K, 3 axes, n, 3 channels), n = nx = ny = nz"""
    return np.stack([j.sum((1, 2)), j.sum((1, 3)), j.sum((2, 3))], 1)


def check_case(j, t, ref, rt, what):
    """K batches (j, t) against the K batches (ref, rt) of the reference: every compared cell under the bar; the detected weight, the detected
    paths and weight x length within 4 sigma; the 3 x 4 x 3 slab sums, each a per-batch total, within 4 sigma; no disagreement, no ended path.
    Compared are the cells the reference fills (a gate that ends at the path length 3.5 leaves the slab farthest from the detector dark, and
    a corner may stay empty in one seed: what the GPU puts there is in the slab sums and the totals, which take every cell); they must be at
    least two thirds of the grid.  Prints the reference's power: the relative standard deviation of the mean per compared cell
    and per slab.  Returns (compared cells, cells beyond 4 sigma, max z, largest total z, largest slab z)"""
    k = len(ref)
    assert j.shape == ref.shape and np.all(t[:, 0] == rt[:, 0]) and np.all(t[:, 12] == 0) and np.all(t[:, 7] == 0)
    on = ref.mean(0) > 0
    assert 3 * on.sum() >= 2 * on.size, "the reference must fill the grid"
    j, ref, full, rfull = j[:, on], ref[:, on], j, ref
    rm = ref.mean(0)
    rel = ref.std(0, ddof=1) / np.sqrt(k) / rm
    sr = slabs(rfull); srel = sr.std(0, ddof=1) / np.sqrt(k) / sr.mean(0)
    print("%s: %d of %d cells compared; reference's relative sd of the mean per cell: median %.3f, max %.3f; per slab: median %.4f, max %.4f" % (what, on.sum(), on.size, np.median(rel), rel.max(), np.median(srel), srel.max()))
    z = S.bar(j.mean(0), j.std(0, ddof=1) / np.sqrt(len(j)), rm, ref.var(0, ddof=1) / k, what=what + " cells")
    zt = [S.total_bar(t[:, q], rt[:, q].mean(), rt[:, q].var(ddof=1) / k, what="%s totals[%d]" % (what, q)) for q in (1, 2, 3, 8, 9, 10, 11)]
    sj = slabs(full)
    zs = [S.total_bar(sj[:, a, i, c], sr[:, a, i, c].mean(), sr[:, a, i, c].var(ddof=1) / k, what="%s slab %s %d channel %d" % (what, "xyz"[a], i, c))
          for a in range(3) for i in range(sj.shape[2]) for c in range(3)]
    return int(on.sum()), int((z > 4).sum()), float(z.max()), float(max(zt)), float(max(zs))


@pytest.mark.parametrize("name", list(CASES))
def test_the_gpu_cases_pass_reference_against_reference(name):
    """the condition under which a case may hold the GPU: two seeds of the reference against each other pass every check the GPU is put to.
    Observed (compared cells of 192, of them beyond 4 sigma, max z, largest total z, largest slab z): ramp, forward 189, 0, 2.93, 0.63, 2.27;
    ramp, back-scatter 192, 0, 3.02, 0.94, 1.66; ramp, side, cone and gate 192, 0, 2.29, 1.06, 1.74; ramp with albedo grid 192, 0, 2.11, 1.01,
    1.45; maximum (strong chroma; further pairs of seeds: 162, 0, 2.46, 0.73, 2.04 and 156, 0, 2.57, 1.43, 2.41) 156, 0, 3.06, 2.82, 3.08;
    single 192, 0, 2.52, 2.99, 3.23.  The relative standard deviation of the mean of a cell: median 0.05 ... 0.16, up to 1 (a cell one
    path reached); of a slab sum: median 0.009 ... 0.017"""
    a, b = case_ref(name, 1), case_ref(name, 0)
    print(name, check_case(a[0], a[1], b[0], b[1], name + ", seed against seed"))
