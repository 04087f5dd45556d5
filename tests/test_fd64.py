"""tests/fd64.py, the float64 restatement of the frequency-domain recorders (include/mer.h, mer_fluence_fd_create / mer_exitance_fd_create),
pinned by closed forms: the complex Beer-Lambert column under an unscattered beam, exact zeros off it, the exact (1, 0) of k = 0, and the
deterministic phase of the beam's exit.  tests/test_gpu_fluence_fd.py and tests/test_gpu_exitance_fd.py hold the GPU against the same closed
forms and against this restatement.  No GPU, no library.

Set-up (tests/test_exitance64.py): the cube [-1, 1]^3, the beam of power 5 from (0.2, 0.1, -3) along +z, K = 16 batches of 16 384 paths,
wavenumbers (0, 0.7, 3.0).  The bar is the project's: totals within 4 sigma, at most 1 + 1 % of the compared values beyond 4 sigma, with the
empirical per-batch variance.  A value is left out of a comparison only when it is exactly 0.0 in every batch on both sides."""
import functools
import numpy as np
from tests import fd64 as F
from tests import test_exitance64 as T

KS = (0.0, 0.7, 3.0)
ABSORBER = 0.8                                 # sigma_a of the pure absorber
COLUMN_RES = (4, 4, 8)                         # the beam's column: ix = 2, iy = 2, eight cells of depth 0.25
COL_IX, COL_IY = 2, 2
# the scattering medium of the GPU comparison
SIGMA_S, SIGMA_A, G, N = 2.0, 0.1, 0.8, 1.4
GRID_RES, MAP_RES = (4, 4, 4), (4, 4)
# the chromatic medium: three different sigma_t under strategy `single`, so that an exit is weighed by tau_c / pdfFailure
CHROMA_S, CHROMA_A = (2.0, 1.5, 1.0), (0.1, 0.2, 0.3)


def absorber_run(n, batches=T.K, seed=31):
    return F.render(T.BEAM, T.POWER, F.Grey(0.0, ABSORBER), 0.0, KS, grid_res=COLUMN_RES, map_res=T.RES, n=n, paths=T.PATHS, batches=batches, seed=seed)


def column_closed_form(n):
    """(n_freq, 2, 8): the expected raw sums per batch of the column's cells"""
    edges = np.arange(9) * 0.25
    ref = np.zeros((len(KS), 2, 8))
    for j, k in enumerate(KS):
        v = T.PATHS * F.absorber_column(T.POWER, ABSORBER, n, k, edges[:-1], edges[1:])
        ref[j, 0], ref[j, 1] = v.real, v.imag
    return ref


def compared(a, b):
    """the mask of the values a comparison keeps: everything that is not exactly 0.0 in every batch on both sides"""
    return ~(np.all(a == 0.0, axis=0) & np.all(b == 0.0, axis=0))


def check_column(grid, n, what):
    """grid: raw sums (K, n_freq, 2, 8, 4, 4) of one channel.  The column against its closed form under the bar; exact zeros elsewhere"""
    k_ = len(grid)
    on = np.zeros(grid.shape[1:], bool); on[:, :, :, COL_IY, COL_IX] = True
    assert np.all(grid[:, ~on] == 0.0), what + ": deposits off the beam's column"
    assert np.all(grid[:, 0, 1] == 0.0), what + ": the imaginary plane of k = 0"
    col = grid[:, :, :, :, COL_IY, COL_IX]                                    # (K, n_freq, 2, 8)
    ref = column_closed_form(n)
    keep = np.ones(ref.shape, bool); keep[0, 1] = False                      # exactly 0.0 on both sides
    assert np.all(ref[0, 1] == 0.0)
    z = F.bar(col.mean(0)[keep], col.std(0, ddof=1)[keep] / np.sqrt(k_), ref[keep], what=what + " column")
    return float(z.max())


def exit_phase_error(emap, totals, n):
    """emap: raw sums (K, n_freq, 2, 6, 4, 4) of one channel: the beam's cell holds N P (cos, sin)(k (2 + 2 n)); the largest absolute error of
    cos and sin over batches and frequencies.  Every other cell must be exactly 0.0"""
    on = np.zeros(emap.shape[1:], bool); on[:, :, T.BEAM_FACE, T.BEAM_IV, T.BEAM_IU] = True
    assert np.all(emap[:, ~on] == 0.0)
    err = 0.0
    for j, k in enumerate(KS):
        phi = k * (2.0 + 2.0 * n)
        unit = emap[:, j, :, T.BEAM_FACE, T.BEAM_IV, T.BEAM_IU] / (totals[:, 14] * T.POWER)[:, None]
        err = max(err, float(np.abs(unit - np.array([np.cos(phi), np.sin(phi)])).max()))
    return err


def test_absorber_column_and_exit_phase():
    for n in (1.0, 1.4):
        r = absorber_run(n)
        zmax = check_column(r["grid"][..., 0], n, "float64, n %.1f" % n)
        err = exit_phase_error(r["map"][..., 0], r["map_totals"], n)
        print("n %.1f: column max z %.2f, exit-phase error %.2e" % (n, zmax, err))
        assert err <= 1e-12
        t = r["map_totals"]
        assert np.all(t[:, 0] == T.PATHS) and np.all(t[:, 4:14] == 0) and np.all(t[:, 14] > 0)
        # the k = 0 real plane is the steady map: sum + missed + rejected = escaped
        np.testing.assert_allclose(r["map"][:, 0, 0].reshape(T.K, -1).sum(1) + t[:, 4] + t[:, 11], t[:, 1], rtol=1e-12)
        # the grid's totals: nothing is dropped (the column lies in the box), every path is counted
        assert np.all(r["grid_totals"][:, 0] == T.PATHS) and np.all(r["grid_totals"][:, 4:7] == 0)


@functools.lru_cache(maxsize=None)
def scattering_ref(seed=41, batches=T.K):
    """the float64 reference of the scattering medium (grey: one channel), computed once"""
    return F.render(T.BEAM, T.POWER, F.Grey(SIGMA_S, SIGMA_A), G, KS, grid_res=GRID_RES, map_res=MAP_RES, n=N, paths=T.PATHS, batches=batches, seed=seed)


@functools.lru_cache(maxsize=None)
def chromatic_ref(seed=43, batches=T.K):
    """... and of the chromatic one (RGB), strategy `single`: the exit weight is tau_c / pdfFailure"""
    med = F.homogeneous(CHROMA_S, CHROMA_A, strategy="single", weight=1.0)
    return F.render(T.BEAM, T.POWER, med, G, KS, grid_res=GRID_RES, map_res=MAP_RES, n=N, paths=T.PATHS, batches=batches, seed=seed)


def compare(a, ta, b, tb, what, totals):
    """raw sums a (K, ...) and totals ta against b, tb under the bar, both sides with their empirical variance; returns (values compared, max z)"""
    ka, kb = len(a), len(b)
    keep = compared(a, b)
    z = F.bar(a.mean(0)[keep], a.std(0, ddof=1)[keep] / np.sqrt(ka), b.mean(0)[keep], b.var(0, ddof=1)[keep] / kb, what=what)
    for q in totals:
        F.total_bar(ta[:, q], tb[:, q].mean(), tb[:, q].var(ddof=1) / kb, what="%s totals[%d]" % (what, q))
    return int(keep.sum()), float(z.max())


def test_two_reference_runs_agree_in_the_scattering_medium():
    """the comparison the GPU tests make, reference against reference: two independent runs of 8 batches"""
    a, b = scattering_ref(seed=41, batches=8), scattering_ref(seed=42, batches=8)
    n_grid, _ = compare(a["grid"], a["grid_totals"], b["grid"], b["grid_totals"], "grid", (1,))
    n_map, _ = compare(a["map"], a["map_totals"], b["map"], b["map_totals"], "map", (1, 14))
    # the only values left out are the imaginary planes of k = 0
    assert n_grid == 384 - 64 and n_map == 576 - 96
    assert np.all(a["grid"][:, 0, 1] == 0.0) and np.all(a["map"][:, 0, 1] == 0.0)
    # the modulus never exceeds the steady sum of the same paths
    for key in ("grid", "map"):
        s = a[key]
        assert np.all(np.hypot(s[:, :, 0], s[:, :, 1]) <= s[:, :1, 0] * (1 + 1e-12))
