"""tests/lightpath64.py, the float64 restatement of the light-path walk with an RGB throughput, pinned by the GREY references that were in the
tree before it: Russian roulette and every distance-sampling strategy are unbiased per channel, so channel c of a chromatic homogeneous
render equals, in expectation, tests/fluence64.py / fluence_time64.py / fluence_track64.py / exitance64.py run grey with sigma_s[c],
sigma_a[c] and power[c].  Those references know nothing of the spectral weighting.  The sigma_t ramp is pinned by closed forms and by the
energy balance.  tests/test_gpu_lightpath_media.py holds the GPU to the same grey references and to this restatement, through the checks
of this module.  No GPU, no library.

Set-up (tests/test_fluence64.py): the cube [-1, 1]^3, the beam from (0.2, 0.1, -3) along +z with the power (5, 3, 8), K = 16 batches of
16 384 paths, g = 0.6; the 8 x 8 x 8 grid, the time grid SC of tests/test_fluence_time64.py, maps of 4 x 4 cells per face, steady and
timed (TMAP).  Statistics: the project's bar -- at most 1 + 1 % of the cells beyond 4 sigma, totals within 4 sigma.

The coefficients are CHROMA / CASES below; what the restatement gives against the grey references (cells beyond 4 sigma per channel) is
printed by every test and recorded in the tests' docstrings."""
import functools
import numpy as np
import pytest
from tests import fluence64 as F
from tests import fluence_time64 as FT
from tests import fluence_track64 as FK
from tests import exitance64 as E
from tests import lightpath64 as LP
from tests import test_fluence64 as T
from tests.test_fluence_time64 import SC

PATHS, K = T.PATHS, T.K
POWER3 = (5.0, 3.0, 8.0)
G = 0.6
CHROMA = {"strong": dict(sigma_s=(2.0, 1.2, 0.6), sigma_a=(0.25, 0.5, 0.1)),
          "medium": dict(sigma_s=(2.0, 1.5, 1.0), sigma_a=(0.25, 0.4, 0.15)),
          "mild": dict(sigma_s=(2.0, 1.8, 1.6), sigma_a=(0.25, 0.3, 0.2))}
# strategy -> coefficients.  `single` with the strong chroma is not used: its per-bounce weight reaches sigma_s,c / rho = 2.9 and the batch
# spreads stop being Gaussian (26 of 512 cells beyond 4 sigma, reference against reference).
CASES = {"balance": "strong", "maximum": "strong", "single": "mild"}
# The time grid under `maximum` takes the medium chroma: with the strong one the late frames of channel 0 (sigma_t 2.25, drawn from the
# 0.7 exponential there) hold few heavy deposits, and lightpath64 against the grey reference put 4, 2 and 6 of 384 bins beyond 4 sigma in
# three seeds (the cap is 4); with the medium chroma 0 0 0 in two seeds, max z 3.96.
TGRID_CASES = {"balance": "strong", "maximum": "medium", "single": "mild"}
GRID = dict(res=T.RES)
MAP = dict(res=(4, 4))
TMAP = dict(res=(4, 4), frames=3, t_min=2.0, t_bin=1.0, cos_min=0.3)      # the exterior leg is 2 and the unscattered beam leaves at 4: the window 2 ... 5 cuts the tail
RAMP = dict(s_lo=0.5, s_hi=4.0, albedo=(0.9, 0.6, 0.3))
RAMP_SEEDS = (41, 42)


def beam(c=None):
    """the beam's geometry; c: with the power of channel c, for a grey reference"""
    return F.collimated([0.2, 0.1, -3.0], [0, 0, 1], 1.0 if c is None else POWER3[c])


@functools.lru_cache(maxsize=None)
def chroma_ref(strategy, part="main"):
    """lightpath64 on the homogeneous chromatic medium of `strategy`, computed once.  part = main: the collision grid, the steady map and,
    where it shares the coefficients, the time grid, all in one walk; tmap: the timed map; tgrid: the time grid; track: the track-length grid
    (single only; a walk of its own because cutting every flight at the cell faces takes several seconds)"""
    seed = {"balance": 51, "maximum": 52, "single": 53}[strategy] + {"main": 0, "tmap": 10, "tgrid": 20, "track": 30}[part]
    kw = dict(paths=PATHS, batches=K, seed=seed)
    if part == "tgrid":
        return LP.render(beam(), POWER3, LP.homogeneous(strategy=strategy, **CHROMA[TGRID_CASES[strategy]]), G, tgrid=SC, **kw)
    med = LP.homogeneous(strategy=strategy, **CHROMA[CASES[strategy]])
    if part == "tmap":
        return LP.render(beam(), POWER3, med, G, emap=TMAP, **kw)
    if part == "track":
        return LP.render(beam(), POWER3, med, G, track=GRID, **kw)
    return LP.render(beam(), POWER3, med, G, grid=GRID, emap=MAP, tgrid=SC if TGRID_CASES[strategy] == CASES[strategy] else None, **kw)


def tgrid_ref(strategy):
    return chroma_ref(strategy, "main" if TGRID_CASES[strategy] == CASES[strategy] else "tgrid")


@functools.lru_cache(maxsize=None)
def grey_ref(chroma, c, what):
    """the grey references run with channel c's numbers, computed once; what = grid / tgrid / emap / tmap / track: (sums, totals)"""
    ss, sa = CHROMA[chroma]["sigma_s"][c], CHROMA[chroma]["sigma_a"][c]
    seed = 100 + 10 * c + (0 if chroma == "strong" else 5)
    kw = dict(paths=PATHS, batches=K, rr_depth=5)
    if what == "grid":
        return F.render(beam(c), ss, sa, G, T.RES, seed=seed, **kw)
    if what == "tgrid":
        return FT.render(beam(c), ss, sa, G, seed=seed + 1, **SC, **kw)
    if what == "emap":
        return E.render(beam(c), ss, sa, G, E.CUBE, MAP["res"], seed=seed + 2, **kw)
    if what == "tmap":
        return E.render(beam(c), ss, sa, G, E.CUBE, **TMAP, seed=seed + 3, **kw)
    assert what == "track"
    return FK.render(beam(c), ss, sa, G, T.RES, seed=seed + 4, **kw)


def _cells(a, r, what):
    """K batches a against K batches r, per cell within the bar with both batch spreads; returns the count beyond 4 sigma and the largest z"""
    z = F.bar(a.mean(0), a.std(0, ddof=1) / np.sqrt(len(a)), r.mean(0), r.var(0, ddof=1) / len(r), what=what)
    return int((z > 4).sum()), float(z.max())


def _total(a, r, what):
    return F.total_bar(a, r.mean(), r.var(ddof=1) / len(r), what=what)


# which totals of a kind are compared (index, name)
TOTALS = {"grid": ((1, "escaped"),), "tgrid": ((1, "escaped"), (8, "out of window")), "track": ((1, "escaped"),),
          "emap": ((1, "escaped"),), "tmap": ((1, "escaped"), (8, "late"), (11, "rejected"))}


def check_against_grey(out, chroma, kinds, what, channels=(0, 1, 2)):
    """`out` (lightpath64.render's dict, or the GPU's results in the same form; a timed map under the key "emap" is named by kinds = ("tmap",)):
    every channel's cells and totals against the grey reference of that channel.  Returns {(kind, c): (cells beyond 4 sigma, max z, total z's)}"""
    res = {}
    for kind in kinds:
        key = "emap" if kind == "tmap" else kind
        for c in channels:
            r, rt = grey_ref(chroma, c, kind)[:2]
            n, zmax = _cells(out[key][..., c], r, "%s %s channel %d against grey" % (what, kind, c))
            zt = [_total(out[key + "_totals"][:, q + c], rt[:, q], "%s %s channel %d %s against grey" % (what, kind, c, name)) for q, name in TOTALS[kind]]
            res[(kind, c)] = (n, zmax, zt)
    return res


def check_against(out, ref, kinds, what):
    """the same, against another render of the same form (the GPU against lightpath64, or two seeds of lightpath64)"""
    for kind in kinds:
        key = "emap" if kind == "tmap" else kind
        for c in range(3):
            _cells(out[key][..., c], ref[key][..., c], "%s %s channel %d against lightpath64" % (what, kind, c))
            for q, name in TOTALS[kind]:
                a, r = out[key + "_totals"][:, q + c], ref[key + "_totals"][:, q + c]
                if r.any() or a.any():
                    _total(a, r, "%s %s channel %d %s against lightpath64" % (what, kind, c, name))


def check_balance(sums, totals, sigma_a, what, extra=None):
    """per channel: sigma_a,c (sum of the cells + dropped [+ extra: the out-of-window weight]) + escaped = paths power_c within 4 sigma"""
    zs = []
    for c in range(3):
        dep = sums[..., c].reshape(len(sums), -1).sum(1) + totals[:, 4 + c] + (0 if extra is None else extra[:, c])
        zs.append(F.total_bar(sigma_a[c] * dep + totals[:, 1 + c], PATHS * POWER3[c], what="%s balance channel %d" % (what, c)))
    return zs


def check_channels_differ(col, what):
    """col (K, n, 3): the beam's column.  The three channels differ pairwise by more than 10 sigma somewhere: one channel recorded three
    times cannot pass"""
    m = col.mean(0); v = col.var(0, ddof=1) / len(col)
    for a, b in ((0, 1), (0, 2), (1, 2)):
        z = np.abs(m[:, a] - m[:, b]) / np.sqrt(v[:, a] + v[:, b])
        print("%s: channels %d and %d differ by up to %.0f sigma" % (what, a, b, z.max()))
        assert z.max() > 10, (what, a, b, z.max())


def column(sums):
    """the beam's column (x = 0.2, y = 0.1) of a (K, nz, ny, nx, 3) grid over the cube: (K, nz, 3)"""
    ny, nx = sums.shape[2:4]
    return sums[:, :, int(np.floor(1.1 / 2 * ny)), int(np.floor(1.2 / 2 * nx)), :]


# ---- chromatic homogeneous media ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strategy", ["balance", "maximum", "single"])
def test_every_channel_is_its_grey_render(strategy):
    """the collision grid (512 cells), the steady map (96) and the time grid (384 bins; under maximum with the medium chroma, TGRID_CASES)
    per channel against the grey reference of that channel; the caps are 6, 1 and 4.  Observed, cells beyond 4 sigma in channels 0 1 2:
    balance grid 1 0 0 (max z 4.49), map 0 1 0 (4.13), time grid 0 0 0; maximum grid 0 0 1 (4.53), map 0 0 0, time grid 0 1 0 (5.34);
    single (mild) 0 0 0 in all three.  The escaped and out-of-window totals: z <= 2.2."""
    out = chroma_ref(strategy)
    chroma = CASES[strategy]
    res = check_against_grey(out, chroma, ("grid", "emap"), strategy)
    tout = tgrid_ref(strategy)
    res.update(check_against_grey(tout, TGRID_CASES[strategy], ("tgrid",), strategy))
    print(strategy, {k: v[:2] for k, v in res.items()}, "largest total z %.2f" % max(max(v[2]) for v in res.values()))
    sa = CHROMA[chroma]["sigma_a"]
    check_balance(out["grid"], out["grid_totals"], sa, strategy + " grid")
    check_balance(tout["tgrid"], tout["tgrid_totals"], CHROMA[TGRID_CASES[strategy]]["sigma_a"], strategy + " time grid", extra=tout["tgrid_totals"][:, 8:11])
    # the collision weights are the absorbed power, and every escaping path is in the map
    np.testing.assert_allclose(out["absorbed"], np.asarray(sa) * out["grid"].reshape(K, -1, 3).sum(1), rtol=1e-9)
    np.testing.assert_allclose(out["emap"].reshape(K, -1, 3).sum(1), out["emap_totals"][:, 1:4], rtol=1e-12)
    assert np.all(out["grid_totals"][:, 4:8] == 0) and np.all(out["grid_totals"][:, 0] == PATHS)
    check_channels_differ(column(out["grid"]), strategy)


@pytest.mark.parametrize("c", [0, 1, 2])
def test_track_grid_channel_is_its_grey_render(c):
    """the track-length grid under single (mild chroma), one channel per case (a grey track reference takes 5 s).  Observed: at most 1 of
    512 cells beyond 4 sigma, max z 4.5"""
    out = chroma_ref("single", "track")
    check_against_grey(out, "mild", ("track",), "single", channels=(c,))
    if c == 0:
        check_balance(out["track"], out["track_totals"], CHROMA["mild"]["sigma_a"], "single track grid")
        check_channels_differ(column(out["track"]), "single track")


@pytest.mark.parametrize("strategy", ["balance", "maximum", "single"])
def test_timed_map_with_a_cone(strategy):
    """the map of TMAP (3 frames of width 1 from t = 2, cos_min = 0.3): cells, escaped, late and rejected per channel against the grey
    reference.  Observed: 0 of 288 keys beyond 4 sigma in every channel but one (single, channel 1: 1, z 5.9; the cap is 3); late and
    rejected z <= 1.2."""
    out = chroma_ref(strategy, "tmap")
    check_against_grey(out, CASES[strategy], ("tmap",), strategy)
    t = out["emap_totals"]
    assert np.all(t[:, 8:11] > 0) and np.all(t[:, 11:14] > 0)
    for c in range(3):
        np.testing.assert_allclose(out["emap"][..., c].reshape(K, -1).sum(1) + t[:, 4 + c] + t[:, 8 + c] + t[:, 11 + c], t[:, 1 + c], rtol=1e-12)


def test_medium_sampling_weight_below_one_balances():
    """grey, medium_sampling_weight = 0.7: 30 % of the flights run to the boundary without sampling the medium; pdfSuccess and pdfFailure
    carry the weight, so escaped + absorbed = emitted, and the cells are those of the analog grey render"""
    out = msw_ref()
    sa = (T.SIGMA_A,) * 3
    check_balance(out["grid"], out["grid_totals"], sa, "weight 0.7")
    r, rt = F.render(beam(0), T.SIGMA_S, T.SIGMA_A, G, T.RES, paths=PATHS, batches=K, seed=61, rr_depth=5)
    _cells(out["grid"][..., 0], r, "weight 0.7 cells against grey")
    _total(out["grid_totals"][:, 1], rt[:, 1], "weight 0.7 escaped against grey")


@functools.lru_cache(maxsize=None)
def msw_ref():
    med = LP.homogeneous((T.SIGMA_S,) * 3, (T.SIGMA_A,) * 3, "single", weight=0.7)
    return LP.render(beam(), POWER3, med, G, grid=GRID, emap=MAP, paths=PATHS, batches=K, seed=60)


# ---- the sigma_t ramp ----------------------------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def ramp_ref(seed, absorbing=False):
    med = LP.ramp(RAMP["s_lo"], RAMP["s_hi"], (0.0,) * 3 if absorbing else RAMP["albedo"])
    return LP.render(beam(), POWER3, med, G, grid=GRID, tgrid=SC, emap=MAP, track=GRID, paths=PATHS, batches=K, seed=seed)


@functools.lru_cache(maxsize=None)
def ramp_albedo_grid_ref():
    """the ramp with the RGB albedo grid of tests/scenes.py (8^3 nodes, values in 0.5 ... 0.95): the collision grid and what escapes"""
    from tests import scenes
    return LP.render(beam(), POWER3, LP.ramp(RAMP["s_lo"], RAMP["s_hi"], scenes.rgb_albedo(8).astype(np.float64)), G, grid=GRID, paths=PATHS, batches=K, seed=43)


def check_absorbing_ramp(out, what):
    """albedo 0: first collisions only.  The column of the collision grid and of the track grid against P integral exp(-tau) over the cell's
    depths under the batch spread, every other cell exactly 0, the escaped weight against P exp(-4.5) -- the integral of sigma_t over the
    beam's chord -- under the binomial variance"""
    med = LP.ramp(RAMP["s_lo"], RAMP["s_hi"], 0.0)
    on, a, b = FK.column_depths(beam(), T.RES)
    assert abs(LP.ramp_depth(med, 2.0) - 4.5) < 1e-12
    pe = np.exp(-4.5)
    for c in range(3):
        mean = PATHS * LP.ramp_column_mean(POWER3[c], med, a, b)
        for key in ("grid", "track"):
            s = out[key][..., c]
            assert np.all(s[:, ~on] == 0.0), "deposits off the beam's column"
            col = s[:, on]
            F.bar(col.mean(0), col.std(0, ddof=1) / np.sqrt(K), mean, what="%s absorbing ramp %s column channel %d" % (what, key, c))
        esc = out["grid_totals"][:, 1 + c]
        z = abs(esc.mean() - PATHS * POWER3[c] * pe) / np.sqrt(PATHS * POWER3[c] ** 2 * pe * (1 - pe) / K)
        print("%s absorbing ramp escaped channel %d: z %.2f" % (what, c, z))
        assert z <= 4


def test_absorbing_ramp_is_the_closed_form():
    out = ramp_ref(40, absorbing=True)
    check_absorbing_ramp(out, "lightpath64")
    np.testing.assert_allclose(out["absorbed"] + out["escaped"], PATHS * np.asarray(POWER3)[None, :].repeat(K, 0), rtol=1e-12)


def test_scattering_ramp_two_seeds_agree_and_balance():
    """Observed, seed against seed: at most 1 cell of 512 beyond 4 sigma per channel in the collision and track grids, 0 of 96 in the map."""
    a, b = ramp_ref(RAMP_SEEDS[0]), ramp_ref(RAMP_SEEDS[1])
    check_against(b, a, ("grid", "tgrid", "track", "emap"), "ramp, seed against seed")
    assert (a["grid"].mean(0) > 0).all() and (a["track"].mean(0) > 0).all()          # every cell is lit
    for c in range(3):
        F.total_bar(a["absorbed"][:, c] + a["escaped"][:, c], PATHS * POWER3[c], what="ramp balance channel %d" % c)
    check_channels_differ(column(a["grid"]), "ramp")


def test_ramp_with_an_albedo_grid_balances():
    """absorbed + escaped = emitted per channel, the absorbed power summed at the collisions with the interpolated albedo"""
    out = ramp_albedo_grid_ref()
    for c in range(3):
        F.total_bar(out["absorbed"][:, c] + out["escaped"][:, c], PATHS * POWER3[c], what="albedo grid balance channel %d" % c)
    assert np.all(out["escaped"] < PATHS * np.asarray(POWER3))
