"""The track-length fluence grid (mer_fluence_track_create, mer_fluence_track.hpp) on the GPU: against closed forms (the analog absorber's
column with its closed-form variance, a clear medium's exact power x length, the erf profile of a sigma_t ramp), against the float64
restatement tests/fluence_track64.py per cell, against the project's own collision grid, the walk against the collision handle's (counters
and totals), along curved rays in a clear gradient-index medium against a float64 trace, and the interface: shards, clear / accumulate, the
bounds-checking build, the refusals, `mer_render --fluence --track-length`.

Set-up: tests/test_gpu_fluence.py's -- 16 384 paths per batch, K = 16 batches with seeds s0 + j, the cube [-1, 1]^3, the beam of power 5 from
(0.2, 0.1, -3) along +z, an 8^3 grid unless said otherwise, medium_sampling_weight = 1.  The seeds of the scattering scenes are the ones
tests/test_gpu_fluence.py uses: the walk is the same, so no path ends by "no forward progress" with them either."""
import functools
import os
import subprocess
import ctypes as C
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host, volio
from tests import fluence64 as F
from tests import fluence_track64 as FT
from tests import test_fluence64 as T
from tests import test_fluence_track64 as TT
from tests import test_gpu_fluence as TG
from tests import test_gpu_ptracer as TP

pytestmark = pytest.mark.gpu
ROOT = TG.ROOT
K, PATHS, SPP, CUBE, RTOL_SUM = TG.K, TG.PATHS, TG.SPP, TG.CUBE, TG.RTOL_SUM
ST = T.SIGMA_S + T.SIGMA_A
CUT_BOX = (T.CUT["bmin"], T.CUT["bmax"])
_base, _absorber, _grey = TG._base, TG._absorber, TG._grey


def _batches(ctx, p, seed0, res=T.RES, box=CUBE, k=K):
    """TG._batches with a track-length handle: raw sums (k, nz, ny, nx, 3), totals (k, 8)"""
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.fluence_track_create(res, box[0], box[1])
    sums, totals = [], []
    try:
        for j in range(k):
            ctx.fluence_clear(h)
            ctx.render_fluence(sc, h, 0, SPP, seed=seed0 + j)
            s, t = ctx.fluence_read(h)
            assert np.isfinite(s).all() and np.isfinite(t).all()
            sums.append(s); totals.append(t)
    finally:
        ctx.fluence_destroy(h)
        for v in vols:
            v.destroy()
    return np.array(sums), np.array(totals)


_CACHE = {}


def _scattering(ctx):
    """the scattering medium on the cube's 8^3 grid, seeds 300 ...: rendered once"""
    if "cube" not in _CACHE:
        _CACHE["cube"] = _batches(ctx, _base(), 300)
    return _CACHE["cube"]


def _grid(**kw):
    """a gridded sigma_t over the cube"""
    base = dict(sigma_mode=P.SIGMA_GRID, density=np.ones((16, 16, 16), np.float32), density_scale=ST, albedo=[T.SIGMA_S / ST] * 3)
    base.update(kw)
    return _base(**base)


def _clear(**kw):
    """no extinction anywhere: a 2^3 density grid of zeros"""
    return _grid(density=np.zeros((2, 2, 2), np.float32), density_scale=1.0, albedo=[0.0] * 3, **kw)


@functools.lru_cache(maxsize=None)
def _ref(which):
    """the float64 references, computed once"""
    if which == "cube":
        return FT.render(T.BEAM, T.SIGMA_S, T.SIGMA_A, T.G, T.RES, paths=PATHS, batches=K, seed=11, rr_depth=5)
    return FT.render(T.BEAM, T.SIGMA_S, T.SIGMA_A, T.G, paths=PATHS, batches=K, seed=12, rr_depth=5, **T.CUT)


# ---- 1. closed forms -------------------------------------------------------------------------------------------------------------------

def test_pure_absorber_column_has_the_closed_form_mean_and_variance(ctx):
    sums, tot = _batches(ctx, _absorber(), 100)
    TT.absorber_column_check(_grey(sums), T.ABSORBER, PATHS, "track absorber column")
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:] == 0)
    F.total_bar(tot[:, 1], PATHS * T.POWER * np.exp(-2 * T.ABSORBER), what="track absorber escaped")


def test_max_depth_2_keeps_the_first_flights(ctx):
    sums, tot = _batches(ctx, _base(max_depth=2), 200)
    TT.absorber_column_check(_grey(sums), ST, PATHS, "track ballistic column")
    assert np.all(tot[:, 7] == 0)


def test_chromatic_absorber_with_one_sampling_channel(ctx):
    """sigma_a = (1, 1.5, 2), strategy single (rho = 1): channel c against P (e^{-sigma_c a} - e^{-sigma_c b}) / sigma_c"""
    sums, tot = _batches(ctx, _base(sigma_s=[0.0] * 3, sigma_a=list(TT.CHROMATIC), g=0.0, strategy=P.STRATEGY_SINGLE), 150)
    for c, s in enumerate(TT.CHROMATIC):
        TT.mean_column_check(sums[..., c], lambda a, b: FT.beer_mean(T.POWER, s, a, b), PATHS, "track chromatic column, channel %d" % c)
    assert np.all(tot[:, 4:] == 0)


# ---- 2. a clear medium, straight rays --------------------------------------------------------------------------------------------------

def test_clear_medium_holds_power_times_length(ctx):
    """no extinction: deterministic.  Every column cell holds PATHS P 0.25 -- the entry point, the cell planes and 5 x 0.25 are exact in
    float32; rtol 1e-6 allows a few roundings of 6e-8 -- every other cell exactly 0.0, all power escapes.  The collision grid of the same scene
    stays empty: the reason the track-length grid exists."""
    sums, tot = _batches(ctx, _clear(), 10, k=2)
    on, a, b = FT.column_depths(T.BEAM, T.RES)
    g = _grey(sums)
    np.testing.assert_allclose(g[:, on], PATHS * T.POWER * 0.25, rtol=1e-6, atol=0)
    assert on.sum() == 8 and np.all(g[:, ~on] == 0.0)
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 1:4] == PATHS * T.POWER) and np.all(tot[:, 4:8] == 0)
    s0, t0 = TG._batches(ctx, _clear(), 10, k=1)
    assert not s0.any() and np.all(t0[:, 1:4] == PATHS * T.POWER)


# ---- 3. a sigma_t ramp -----------------------------------------------------------------------------------------------------------------

def test_sigma_ramp_follows_the_erf_profile(ctx):
    """a 2 x 2 x 2 density grid, 0 on the z = -1 nodes and 1 on the z = +1 nodes, scale 4, albedo 0: sigma_t = 4 (z + 1) / 2"""
    dens = np.zeros((2, 2, 2), np.float32); dens[1] = 1.0
    sums, tot = _batches(ctx, _grid(density=dens, density_scale=TT.RAMP_MAX, albedo=[0.0] * 3), 250)
    TT.mean_column_check(_grey(sums), lambda a, b: FT.ramp_mean(T.POWER, 1.0, a, b), PATHS, "track ramp column")
    F.total_bar(tot[:, 1], PATHS * T.POWER * np.exp(-4.0), what="track ramp escaped")
    assert np.all(tot[:, 4:] == 0)


# ---- 4. against the float64 restatement ------------------------------------------------------------------------------------------------

def test_scattering_medium_matches_float64(ctx):
    sums, tot = _scattering(ctx)
    TG._against_ref(sums, tot, _ref("cube"), "track cube")


def test_box_that_cuts_the_shape_matches_float64(ctx):
    """a 4 x 6 x 5 grid over (-1, -0.5, -1) ... (0.5, 1, 0.25): a transposed or off-by-one index cannot pass"""
    sums, tot = _batches(ctx, _base(), 400, res=T.CUT["res"], box=CUT_BOX)
    assert sums.shape == (K, 5, 6, 4, 3) and np.all(tot[:, 4] > 0)
    TG._against_ref(sums, tot, _ref("cut"), "track cut")


# ---- 5. against the collision grid -----------------------------------------------------------------------------------------------------

def test_agrees_with_the_collision_grid(ctx):
    """the project's own collision estimator, other seeds: per cell within the bar with both batch spreads; and the equal-paths noise"""
    a, ta = _scattering(ctx)
    b, tb = TG._batches(ctx, _base(), 2300)
    ga, gb = _grey(a), _grey(b)
    F.bar(ga.mean(0), ga.std(0, ddof=1) / np.sqrt(K), gb.mean(0), gb.var(0, ddof=1) / K, what="track vs collision")
    F.total_bar(ta[:, 1], tb[:, 1].mean(), tb[:, 1].var(ddof=1) / K, what="track vs collision escaped")
    rel = (gb.std(0, ddof=1) / gb.mean(0)) / (ga.std(0, ddof=1) / ga.mean(0))
    print("relative batch spread collision / track: median %.2f (variance ratio %.2f), range %.2f ... %.2f" % (np.median(rel), np.median(rel) ** 2, rel.min(), rel.max()))


# ---- 6. the same walk ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["straight homogeneous", "curved gridded"])
def test_same_walk_as_the_collision_grid(ctx, which):
    p = _base() if which == "straight homogeneous" else _grid(rif_mode=P.RIF_TRILINEAR, rif=TG._rif(), stepsize=0.05, stepper=P.STEP_VERLET)
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    got = []
    for create in (ctx.fluence_create, ctx.fluence_track_create):
        h = create(T.RES, *CUBE)
        try:
            ctx.counters_reset()
            ctx.render_fluence(sc, h, 0, SPP, seed=7)
            got.append((ctx.counters(), ctx.fluence_read(h)[1]))
        finally:
            ctx.fluence_destroy(h)
    for v in vols:
        v.destroy()
    (ca, ta), (cb, tb) = got
    print("collision", ca[:8], "track", cb[:8])
    assert ca[capi.C_PATHS] == PATHS and ca[capi.C_REAL] > PATHS
    for c in (capi.C_PATHS, capi.C_SEGMENTS, capi.C_REAL, capi.C_TENTATIVE, capi.C_STEPS):
        assert ca[c] == cb[c], (c, ca[c], cb[c])
    assert ta[0] == tb[0] == PATHS and ta[7] == tb[7]
    np.testing.assert_allclose(tb[1:4], ta[1:4], rtol=RTOL_SUM, atol=0)


# ---- 7. a clear gradient-index medium, curved rays -------------------------------------------------------------------------------------

def _verlet(p, v, h):
    """one velocity-Verlet step of the eikonal equations for n = RIF_A + RIF_B y (float64), in the kernel's order"""
    g = np.array([0.0, TP.RIF_B, 0.0])
    v = v + 0.5 * h * g
    p = p + h * v / (TP.RIF_A + TP.RIF_B * p[1])
    return p, v + 0.5 * h * g


def _coarse_length(stepper, h):
    """the arc length of the beam to the cube's exit, traced in float64 with the kernel's stepper and step h; the last step is shortened by bisection"""
    step = _verlet if stepper == P.STEP_VERLET else TP._rk4
    p = np.array([TG.BEAM_O[0], TG.BEAM_O[1], -1.0]); v = np.array(TG.BEAM_D) * (TP.RIF_A + TP.RIF_B * p[1])
    s = 0.0
    for _ in range(100000):
        q, w = step(p, v, h)
        if np.all(np.abs(q) <= 1):
            p, v, s = q, w, s + h
            continue
        lo, hi = 0.0, h
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if np.all(np.abs(step(p, v, mid)[0]) <= 1):
                lo = mid
            else:
                hi = mid
        return s + lo
    raise AssertionError("the beam never left the cube")


@pytest.mark.parametrize("stepper", [P.STEP_VERLET, P.STEP_RK4])
def test_clear_curved_beam_follows_the_float64_trace(ctx, stepper):
    """n = 1.3 + 0.15 y on a 5^3 dense grid, zero density, stepsize 0.05: per z slab the centroid of the sums lies within half a cell of the
    unweighted mean of the float64 trace in that slab, and the mean deposited length lies in [L - h - e, L + e]: L the trace's arc length, h
    the step (the piece before the boundary that the walk loses), e the difference between L and a float64 trace with the kernel's stepper
    and step"""
    h = 0.05
    pts, s = TG._beam_trace()
    L = s[-1]
    e = abs(L - _coarse_length(stepper, h))
    sums, tot = _batches(ctx, _clear(rif_mode=P.RIF_TRILINEAR, rif=TG._rif(), stepsize=h, stepper=stepper), 700 + stepper, k=4)
    g = _grey(sums).sum(0)
    centres = -1 + (np.arange(8) + 0.5) * 0.25
    worst = 0.0
    for kz in range(8):
        slab = g[kz]
        assert slab.sum() > 0
        cy = (slab.sum(1) * centres).sum() / slab.sum(); cx = (slab.sum(0) * centres).sum() / slab.sum()
        m = (pts[:, 2] >= -1 + 0.25 * kz) & (pts[:, 2] < -1 + 0.25 * (kz + 1))
        worst = max(worst, abs(cy - pts[m, 1].mean()), abs(cx - pts[m, 0].mean()))
    length = _grey(sums).sum() / (len(sums) * PATHS * T.POWER)
    print("stepper %d: L %.5f, e %.2e, mean deposited length %.5f, largest centroid offset %.4f" % (stepper, L, e, length, worst))
    assert worst <= 0.125
    assert L - h - e <= length <= L + e
    assert np.all(tot[:, 1:4] == PATHS * T.POWER) and np.all(tot[:, 4:] == 0)


# ---- 8. gridded sigma_t, curved scattering ---------------------------------------------------------------------------------------------

def test_gridded_sigma_matches_homogeneous(ctx):
    a, ta = _batches(ctx, _grid(), 500)
    b, tb = _batches(ctx, _base(), 600)
    ga, gb = _grey(a), _grey(b)
    F.bar(ga.mean(0), ga.std(0, ddof=1) / np.sqrt(K), gb.mean(0), gb.var(0, ddof=1) / K, what="track grid vs homogeneous")
    F.total_bar(ta[:, 1], tb[:, 1].mean(), tb[:, 1].var(ddof=1) / K, what="track grid escaped")
    F.total_bar(T.SIGMA_A * ga.sum((1, 2, 3)) + ta[:, 1], PATHS * T.POWER, what="track grid balance")
    assert np.all(ta[:, 7] == 0)


@pytest.mark.parametrize("stepper", [P.STEP_VERLET, P.STEP_RK4])
def test_curved_scattering_balances(ctx, stepper):
    """absorbed + escaped = emitted in expectation along curved rays; the seeds of tests/test_gpu_fluence.py, for which totals[7] == 0.
    The stepsize: an escaping flight deposits nothing for the step that left the shape (mer.h), so it loses at most h of path, h / 2 on
    average, and the balance falls short by about sigma_a h / 2 x the escaped fraction.  Measured at h = 0.05, as the collision grid's test
    has it: mean / emitted = 0.9966 (Verlet, z 3.81) and 0.9968 (RK4, z 4.17) -- 0.25 x 0.025 x the 0.60 that escapes predicts 0.0038
    short: the loss the header documents, at the edge of the bar with these 262 144 paths.  The balance is therefore checked at h = 0.01,
    where the same loss is 0.0007 of the emitted power, below the 0.0009 that one standard error of the total is (measured: 0.9995 and
    0.9997, z 0.57 and 0.38); a lost or doubled cell still fails it."""
    sums, tot = _batches(ctx, _base(rif_mode=P.RIF_TRILINEAR, rif=TG._rif(), stepsize=0.01, stepper=stepper), 1000 + stepper)
    assert np.all(tot[:, 7] == 0) and np.all(tot[:, 4:7] == 0)
    F.total_bar(T.SIGMA_A * _grey(sums).sum((1, 2, 3)) + tot[:, 1], PATHS * T.POWER, what="track curved balance")


# ---- 9. the interface ------------------------------------------------------------------------------------------------------------------

def test_half_shards_add_up_and_the_grid_accumulates(ctx):
    sc, _ = ctx.upload_scene(_base())
    h = ctx.fluence_track_create(T.RES, *CUBE)
    try:
        ctx.render_fluence(sc, h, 0, SPP, seed=9)
        whole, tw = ctx.fluence_read(h)
        parts = []
        for begin in (0, 32):
            ctx.fluence_clear(h)
            z, tz = ctx.fluence_read(h)
            assert not z.any() and not tz.any()
            ctx.render_fluence(sc, h, begin, 32, seed=9)
            parts.append(ctx.fluence_read(h))
        assert parts[0][1][0] == parts[1][1][0] == PATHS // 2 and tw[0] == PATHS
        assert parts[0][0].sum() > 0 and not np.array_equal(parts[0][0], parts[1][0])
        np.testing.assert_allclose(parts[0][0] + parts[1][0], whole, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(parts[0][1] + parts[1][1], tw, rtol=RTOL_SUM, atol=0)
        ctx.render_fluence(sc, h, 0, 32, seed=9)
        both, tb = ctx.fluence_read(h)
        np.testing.assert_allclose(both, whole, rtol=RTOL_SUM, atol=0)
        assert tb[0] == PATHS
        # a steady-state grid: the time-resolved reader refuses it, in the front end and in the library
        with pytest.raises(capi.MerError, match="steady-state grid: use mer_fluence_read"):
            ctx.fluence_time_read(h)
        t12 = np.zeros(12)
        assert ctx.lib.mer_fluence_time_read(ctx.h, C.c_int32(h), None, t12.ctypes.data_as(C.c_void_p)) != 0
        assert "steady-state grid: use mer_fluence_read" in ctx.lib.mer_last_error(ctx.h).decode()
    finally:
        ctx.fluence_destroy(h)


def test_bounds_checking_build_agrees(ctx):
    """libmer_check.so: a straight gridded scene and a curved scene with the box that cuts the cube form no index outside a device buffer, and
    give the product build's sums"""
    cases = (_grid(), _base(rif_mode=P.RIF_TRILINEAR, rif=TG._rif(), stepsize=0.05, stepper=P.STEP_VERLET))
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for p in cases:
            got = []
            for cx in (c, ctx):
                sc, vols = cx.upload_scene(p, layout=capi.LAYOUT_DENSE)
                phi, info = cx.fluence(sc, T.CUT["res"], SPP, seed=3, bmin=T.CUT["bmin"], bmax=T.CUT["bmax"], estimator="track")
                assert info["estimator"] == "track"
                got.append((info["sums"], info))
                for v in vols:
                    v.destroy()
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (n, kind, idx, lim)
            assert got[0][0].sum() > 0 and got[0][1]["dropped"][0] > 0
            np.testing.assert_allclose(got[0][0], got[1][0], rtol=RTOL_SUM, atol=0)
            assert got[0][1]["paths"] == got[1][1]["paths"] == PATHS
    finally:
        c.close()


def test_refuses_distance_sampling_that_is_not_analog(ctx):
    """balance with a chromatic sigma_t, medium_sampling_weight 0.8 and maximum: refused for a track-length handle, by name, before any launch;
    a collision handle still renders the same scenes"""
    ht = ctx.fluence_track_create(T.RES, *CUBE)
    hc = ctx.fluence_create(T.RES, *CUBE)
    chroma = dict(sigma_s=[0.0] * 3, sigma_a=list(TT.CHROMATIC), g=0.0)
    cases = ((_base(**chroma), "strategy balance with a channel-dependent sigma_t"),
             (_base(medium_sampling_weight=0.8), "medium_sampling_weight must be 1"),
             (_base(strategy=P.STRATEGY_MAXIMUM, **chroma), "strategy maximum"))
    try:
        for p, msg in cases:
            sc, _ = ctx.upload_scene(p)
            with pytest.raises(capi.MerError, match="track-length grid needs analog distance sampling.*" + msg):
                ctx.render_fluence(sc, ht, 0, 1)
            ctx.fluence_clear(hc)
            ctx.render_fluence(sc, hc, 0, 1)
            s, t = ctx.fluence_read(hc)
            assert s.sum() > 0 and t[0] == TG.W * TG.H
        s, t = ctx.fluence_read(ht)
        assert not s.any() and not t.any()                                 # nothing was launched
        # balance with three equal sigma_t is analog
        ctx.render_fluence(ctx.upload_scene(_base())[0], ht, 0, 1)
        assert ctx.fluence_read(ht)[0].sum() > 0
        with pytest.raises(capi.MerError, match="estimator must be"):
            ctx.fluence(ctx.upload_scene(_base())[0], T.RES, 1, estimator="expected")
    finally:
        ctx.fluence_destroy(ht); ctx.fluence_destroy(hc)


def test_mer_render_track_length_writes_the_python_calls_grid(ctx, tmp_path):
    """mer_render --fluence=8,8,8 --track-length on scenes/cfg_laser_clear.xml: the grid Context.fluence(..., estimator="track") gives"""
    scene = os.path.join(ROOT, "scenes", "cfg_laser_clear.xml")
    for defines in ({"samples": "1", "sigmaS": "0", "sigmaA": "0"}, {"samples": "1", "sigmaS": "0.8", "sigmaA": "0.05"}):
        out = str(tmp_path / "phi.vol")
        args = [os.path.join(ROOT, "mitsubaer_amd", "mer_render"), "--fluence=8,8,8", "--track-length", "--seed", "3", "-o", out]
        for k, v in defines.items():
            args += ["-D", "%s=%s" % (k, v)]
        r = subprocess.run(args + [scene], capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, r.stderr
        assert "paths %d " % (128 * 96) in r.stdout
        data, lo, hi = volio.read_vol(out, mmap=False)
        assert data.shape == (8, 8, 8, 3) and data.dtype == np.float32
        d, spp = host.flatten_xml(scene, defines)
        phi, info = ctx.fluence(d, (8, 8, 8), spp, seed=3, estimator="track")
        assert info["paths"] == 128 * 96 and info["estimator"] == "track" and phi.sum() > 0
        np.testing.assert_allclose(data, phi.astype(np.float32), rtol=1e-6, atol=0)
        if defines["sigmaS"] == "0":                                       # the clear medium: the collision grid of the same scene is empty
            assert not ctx.fluence(d, (8, 8, 8), spp, seed=3)[0].any()
