"""The time-resolved fluence grid (mer_fluence_time_create, the TIMED instantiations of fluence_kernel in mer_fluence.hpp) on the GPU: against
the closed form of an unscattered pulse per (frame, cell), against the steady-state grid of the same walk, against the float64 restatement
tests/fluence_time64.py per bin, along curved rays against a float64 RK4 trace of the beam that accumulates the optical length, and the
interface: shards, clear / accumulate, the bounds-checking build, the refusals, `mer_render --fluence --time-resolved`.

Set-up (tests/test_gpu_fluence.py, tests/test_fluence_time64.py): a 16 x 16 film (path enumeration only) x 64 samples = 16 384 paths per
batch, K = 16 batches with seeds s0 + j, the cube [-1, 1]^3, the beam of power 5 from (0.2, 0.1, -3) along +z (an exterior leg of 2 at
index 1), medium_sampling_weight = 1.  Statistics: the project's bar -- at most 1 + 1 % of the bins beyond 4 sigma, totals within 4 sigma."""
import os
import re
import subprocess
import ctypes as C
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host
from tests import fluence_time64 as FT
from tests import test_fluence64 as T
from tests import test_fluence_time64 as TT
from tests import test_gpu_fluence as G
from tests import test_gpu_ptracer as TP

pytestmark = pytest.mark.gpu
ROOT = G.ROOT
K, SPP, PATHS, CUBE, RTOL_SUM = G.K, G.SPP, G.PATHS, G.CUBE, G.RTOL_SUM


def _batches(ctx, p, seed0, res, frames, t_min, t_bin, box=CUBE, k=K):
    """k batches with seeds seed0 + j into one time-resolved grid, cleared in between: raw sums (k, frames, nz, ny, nx, 3), totals (k, 12)"""
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.fluence_time_create(res, box[0], box[1], frames, t_min, t_bin)
    sums, totals = [], []
    try:
        for j in range(k):
            ctx.fluence_clear(h)
            ctx.render_fluence(sc, h, 0, SPP, seed=seed0 + j)
            s, t = ctx.fluence_time_read(h)
            assert s.shape == (frames, res[2], res[1], res[0], 3) and t.shape == (12,)
            assert np.isfinite(s).all() and np.isfinite(t).all() and t[11] == 0
            sums.append(s); totals.append(t)
    finally:
        ctx.fluence_destroy(h)
        for v in vols:
            v.destroy()
    return np.array(sums), np.array(totals)


def _grey_totals(tot):
    """a grey scene: the three channels of every weight total hold the same sum"""
    for q in (1, 4, 8):
        np.testing.assert_allclose(tot[:, q + 1], tot[:, q], rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(tot[:, q + 2], tot[:, q], rtol=RTOL_SUM, atol=0)


# ---- 1. the closed form of an unscattered pulse ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("rif_const", TT.RIF_CONSTS)
def test_pure_absorber_is_beer_lambert_per_frame(ctx, rif_const):
    """sigma_a = 1.5, an 8 x 8 x 8 grid with 8 frames from t_min = 1.9 of width 0.35: every (frame, cell) of the beam's column against
    P / sigma_t times Beer-Lambert over the depths the pulse crosses during that frame (frame edges at -0.0714 + 0.25 f for n = 1.4, at
    -0.1 + 0.35 f for n = 1: the factor n and the exterior leg show separately) under the binomial variance; every bin off the column and
    every bin of a frame the closed form excludes exactly 0.0.  Out of the window (n = 1.4): depths behind z* = 2.7 / 1.4, 0.56 % of the
    paths.  totals[8] is a sum of deposit weights P / sigma_t, so sigma_t totals[8] -- the power absorbed outside the window -- is what is
    held to paths P (e^{-1.5 z*} - e^{-3}), by total_bar.  With n = 1 nothing falls outside and totals[8] is exactly 0."""
    sums, tot = _batches(ctx, G._absorber(rif_const=rif_const), 2100 + int(10 * rif_const), **TT.ABS)
    g = G._grey(sums); _grey_totals(tot)
    TT.column_time_check(g, tot[:, 8], T.ABSORBER, rif_const, PATHS, "absorber column, n = %g" % rif_const)
    if rif_const == 1.4:
        assert np.all(tot[:, 8] > 0)
        assert 0.004 < T.ABSORBER * tot[:, 8].sum() / (K * PATHS * T.POWER) < 0.007
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:8] == 0)
    # every path deposits P / sigma_t once, in or out of the window, or escapes with P (a deposit is P tau / pdf in float32)
    np.testing.assert_allclose(T.ABSORBER * (g.sum((1, 2, 3, 4)) + tot[:, 8]) + tot[:, 1], PATHS * T.POWER, rtol=1e-6)


# ---- 2. the sum over the frames is the steady-state grid -------------------------------------------------------------------------------

def test_sum_over_frames_is_the_steady_state_grid(ctx):
    """max_depth = 6: a path length is at most 2 + 5 * 2 sqrt(3) < 32, so 32 frames of width 1 from 0 hold every deposit.  The timed and the
    steady-state kernel walk the same paths: equal counters, equal totals, and the frames add up to the steady-state sums"""
    sc, _ = ctx.upload_scene(G._base(max_depth=6))
    ht = ctx.fluence_time_create(T.RES, CUBE[0], CUBE[1], 32, 0.0, 1.0)
    hs = ctx.fluence_create(T.RES, *CUBE)
    try:
        ctx.counters_reset()
        ctx.render_fluence(sc, ht, 0, SPP, seed=7)
        a = ctx.counters()
        ctx.counters_reset()
        ctx.render_fluence(sc, hs, 0, SPP, seed=7)
        b = ctx.counters()
        st, tt = ctx.fluence_time_read(ht)
        ss, ts = ctx.fluence_read(hs)
    finally:
        ctx.fluence_destroy(ht); ctx.fluence_destroy(hs)
    assert st.shape == (32,) + ss.shape and ss.sum() > 0
    assert not tt[8:].any()
    assert (st.sum((1, 2, 3, 4)) > 0).sum() >= 4                             # the deposits do spread over the frames
    assert not st[:2].any()                                                   # and none comes before the exterior leg is behind it
    np.testing.assert_allclose(st.sum(0), ss, rtol=RTOL_SUM, atol=0)
    assert tt[0] == ts[0] == PATHS and tt[7] == ts[7]
    np.testing.assert_allclose(tt[:8], ts, rtol=RTOL_SUM, atol=0)
    assert a[capi.C_PATHS] == PATHS and a[capi.C_REAL] > PATHS
    for c in (capi.C_PATHS, capi.C_SEGMENTS, capi.C_REAL):
        assert a[c] == b[c], (c, a[c], b[c])


# ---- 3. against the float64 restatement ------------------------------------------------------------------------------------------------

def test_scattering_medium_matches_float64(ctx):
    """the scattering medium on a 4 x 4 x 4 grid with 6 frames from t_min = 2 of width 1: per bin within the bar with both batch spreads,
    the escaped, dropped and out-of-window totals within 4 sigma (tests/test_fluence_time64.py shows the restatement meets this bar
    against itself at this size)"""
    sums, tot = _batches(ctx, G._base(), 2300, **TT.SC)
    _grey_totals(tot)
    TT.against(G._grey(sums), tot, TT.scattering_ref(TT.SC_SEEDS[0]), "gpu vs float64")
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 8] > 0)


# ---- 4. curved rays --------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("stepper", [P.STEP_VERLET, P.STEP_RK4])
def test_curved_beam_is_binned_by_its_optical_length(ctx, stepper):
    """n = 1.3 + 0.15 y on a 5^3 dense grid, stepsize 0.05, a pure absorber, 6 frames of width 0.5 from 1.9.  The beam is traced in float64
    (test_gpu_fluence._beam_trace) and the optical length 2 + integral n ds accumulated along it; with s_a, s_b the arc lengths at which it
    crosses a frame's edges (clipped to the traversal), the fraction of the paths that deposit during that frame is
    e^{-sigma s_a} - e^{-sigma s_b}: binomial z <= 4 per frame"""
    frames, t_min, t_bin = 6, 1.9, 0.5
    pts, s = G._beam_trace()
    n = TP.RIF_A + TP.RIF_B * pts[:, 1]
    opt = 2.0 + np.concatenate([[0.0], np.cumsum(0.5 * (n[1:] + n[:-1]) * np.diff(s))])
    assert t_min < opt[0] and opt[-1] < t_min + frames * t_bin and opt[-1] > t_min + (frames - 1) * t_bin      # the traversal ends in the last frame
    sums, tot = _batches(ctx, G._absorber(rif_mode=P.RIF_TRILINEAR, rif=G._rif(), stepsize=0.05, stepper=stepper), 2400 + stepper,
                         T.RES, frames, t_min, t_bin)
    g = G._grey(sums)
    assert not tot[:, 4:].any()
    worst = 0.0
    for f in range(frames):
        sa, sb = np.interp([t_min + f * t_bin, t_min + (f + 1) * t_bin], opt, s)           # clipped to [0, L] outside the traversal
        pf = np.exp(-T.ABSORBER * sa) - np.exp(-T.ABSORBER * sb)
        frac = T.ABSORBER * g[:, f].sum() / (K * PATHS * T.POWER)
        z = abs(frac - pf) / np.sqrt(pf * (1 - pf) / (K * PATHS))
        print("stepper %d frame %d: arc lengths %.4f ... %.4f, deposited fraction %.6f, closed form %.6f, z %.2f" % (stepper, f, sa, sb, frac, pf, z))
        assert pf > 0.01
        worst = max(worst, z)
    assert worst <= 4


# ---- 5. gridded sigma_t ----------------------------------------------------------------------------------------------------------------

def test_gridded_sigma_matches_homogeneous(ctx):
    """a constant 16^3 density with scale = sigma_t (delta tracking) against the homogeneous medium: per bin within the bar, with both batch
    spreads, and the out-of-window weight within 4 sigma"""
    st = T.SIGMA_S + T.SIGMA_A
    grid = G._base(sigma_mode=P.SIGMA_GRID, density=np.ones((16, 16, 16), np.float32), density_scale=st, albedo=[T.SIGMA_S / st] * 3)
    a, ta = _batches(ctx, grid, 2500, **TT.SC)
    b, tb = _batches(ctx, G._base(), 2600, **TT.SC)
    TT.against(G._grey(a), ta, (G._grey(b), tb), "grid vs homogeneous")


# ---- 6. shards, clear, accumulate ------------------------------------------------------------------------------------------------------

def test_half_shards_add_up_and_the_grid_accumulates(ctx):
    sc, _ = ctx.upload_scene(G._base())
    h = ctx.fluence_time_create(TT.SC["res"], CUBE[0], CUBE[1], TT.SC["frames"], TT.SC["t_min"], TT.SC["t_bin"])
    try:
        ctx.render_fluence(sc, h, 0, SPP, seed=9)
        whole, tw = ctx.fluence_time_read(h)
        parts = []
        for begin in (0, 32):
            ctx.fluence_clear(h)
            z, tz = ctx.fluence_time_read(h)
            assert not z.any() and not tz.any()
            ctx.render_fluence(sc, h, begin, 32, seed=9)
            parts.append(ctx.fluence_time_read(h))
        assert parts[0][1][0] == parts[1][1][0] == PATHS // 2 and tw[0] == PATHS and tw[8] > 0
        assert parts[0][0].sum() > 0 and not np.array_equal(parts[0][0], parts[1][0])
        np.testing.assert_allclose(parts[0][0] + parts[1][0], whole, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(parts[0][1] + parts[1][1], tw, rtol=RTOL_SUM, atol=0)
        # the second half went into a cleared grid; the first half on top of it accumulates to the whole
        ctx.render_fluence(sc, h, 0, 32, seed=9)
        both, tb = ctx.fluence_time_read(h)
        np.testing.assert_allclose(both, whole, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(tb, tw, rtol=RTOL_SUM, atol=0)
        _, t_only = ctx.fluence_time_read(h, sums=False)
        assert np.array_equal(t_only, tb)
    finally:
        ctx.fluence_destroy(h)


# ---- 7. the bounds-checking build ------------------------------------------------------------------------------------------------------

def test_bounds_checking_build_agrees(ctx):
    """libmer_check.so on the cut box with 5 frames: a straight gridded scene and a curved scene form no index outside a device buffer (the
    key frame * cells + cell goes through the check), and give the product build's grids"""
    st = T.SIGMA_S + T.SIGMA_A
    cases = (G._base(sigma_mode=P.SIGMA_GRID, density=np.ones((16, 16, 16), np.float32), density_scale=st, albedo=[T.SIGMA_S / st] * 3),
             G._base(rif_mode=P.RIF_TRILINEAR, rif=G._rif(), stepsize=0.05, stepper=P.STEP_VERLET))
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for p in cases:
            got = []
            for cx in (c, ctx):
                sc, vols = cx.upload_scene(p, layout=capi.LAYOUT_DENSE)
                phi, info = cx.fluence_time(sc, T.CUT["res"], 5, 2.0, 1.0, SPP, seed=3, bmin=T.CUT["bmin"], bmax=T.CUT["bmax"])
                got.append((info["sums"], info))
                for v in vols:
                    v.destroy()
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (n, kind, idx, lim)
            assert got[0][0].shape == (5, 5, 6, 4, 3) and got[0][0].sum() > 0
            assert got[0][1]["dropped"][0] > 0 and got[0][1]["out_of_window"][0] > 0
            np.testing.assert_allclose(got[0][0], got[1][0], rtol=RTOL_SUM, atol=0)
            np.testing.assert_allclose(got[0][1]["out_of_window"], got[1][1]["out_of_window"], rtol=RTOL_SUM, atol=0)
            assert got[0][1]["paths"] == got[1][1]["paths"] == PATHS
    finally:
        c.close()


# ---- 8. refusals past the Python check -------------------------------------------------------------------------------------------------

def test_library_refusals(ctx):
    def last():
        return ctx.lib.mer_last_error(ctx.h).decode()

    def raw(res=(8, 8, 8), lo=(-1, -1, -1), hi=(1, 1, 1), frames=8, t_min=1.9, t_bin=0.35, reserved=0):
        d = capi.fluence_time_desc(res, lo, hi, frames, t_min, t_bin)
        d.reserved = reserved
        return d
    for kw, msg in ((dict(frames=0), "frames must lie in 1 ... 4096"), (dict(frames=4097), "frames must lie in 1 ... 4096"),
                    (dict(t_bin=0.0), "t_bin must be finite and greater than 0"), (dict(t_bin=-1.0), "t_bin must be finite and greater than 0"),
                    (dict(t_bin=float("nan")), "t_bin must be finite and greater than 0"), (dict(t_min=float("inf")), "t_min must be finite"),
                    (dict(reserved=7), "reserved must be 0"), (dict(res=(1024, 1024, 64), frames=3), "more than 2\\^27 cells x frames"),
                    (dict(res=(0, 8, 8)), "res must lie in 1 ... 1024"), (dict(lo=(-1, 1, -1)), "bmin must be below bmax"),
                    (dict(hi=(1, float("nan"), 1)), "bmin / bmax must be finite"), (dict(res=(1024, 1024, 129), frames=1), "more than 2\\^27 cells")):
        out = C.c_int32(-1)
        d = raw(**kw)
        assert ctx.lib.mer_fluence_time_create(ctx.h, C.byref(d), C.byref(out)) != 0 and out.value == 0, kw
        assert re.match("mer_fluence_time_create: .*" + msg, last()), (kw, last())
        with pytest.raises(capi.MerError, match=msg):                        # the Python check says the same
            capi.validate_fluence_time(d)
    ht = ctx.fluence_time_create(T.RES, CUBE[0], CUBE[1], 8, 1.9, 0.35)
    hs = ctx.fluence_create(T.RES, *CUBE)
    try:
        # each kind of handle reads through its own call
        t12 = np.zeros(12); buf = np.zeros((8, 8, 8, 8, 3))
        assert ctx.lib.mer_fluence_read(ctx.h, C.c_int32(ht), None, t12.ctypes.data_as(C.c_void_p)) != 0
        assert "time-resolved grid: use mer_fluence_time_read" in last()
        assert ctx.lib.mer_fluence_time_read(ctx.h, C.c_int32(hs), buf.ctypes.data_as(C.c_void_p), t12.ctypes.data_as(C.c_void_p)) != 0
        assert "use mer_fluence_read" in last() and not buf.any()
        with pytest.raises(capi.MerError, match="use mer_fluence_time_read"):
            ctx.fluence_read(ht)
        with pytest.raises(capi.MerError, match="use mer_fluence_read"):
            ctx.fluence_time_read(hs)
        # unknown handles
        assert ctx.lib.mer_fluence_time_read(ctx.h, C.c_int32(ht + 1000), None, t12.ctypes.data_as(C.c_void_p)) != 0
        assert "mer_fluence_time_read: unknown fluence handle" in last()
        assert ctx.lib.mer_fluence_time_read(ctx.h, C.c_int32(0), None, t12.ctypes.data_as(C.c_void_p)) != 0
        with pytest.raises(capi.MerError, match="unknown fluence handle"):
            ctx.fluence_time_read(ht + 1000)
        # the scene's scope is the steady-state grid's: a volpath scene is refused, and nothing was launched
        sc = ctx.upload_scene(G._base())[0]; sc.integrator = P.INTEGRATOR_VOLPATH
        with pytest.raises(capi.MerError, match="integrator must be ptracer"):
            ctx.render_fluence(sc, ht, 0, 1)
        s, t = ctx.fluence_time_read(ht)
        assert not s.any() and not t.any()
    finally:
        ctx.fluence_destroy(ht); ctx.fluence_destroy(hs)
    with pytest.raises(capi.MerError, match="unknown fluence handle"):       # destroyed: no longer a handle of either kind
        ctx.fluence_time_read(ht)


# ---- 9. the command line ---------------------------------------------------------------------------------------------------------------

def test_mer_render_time_resolved_writes_the_python_calls_grid(ctx, tmp_path):
    """mer_render --fluence=8,8,8 --time-resolved on the laser example, the window from the film (tMin = 4, tMax = 9, tRes = 0.5: 10 frames):
    a float32 .npy [10][8][8][8][3] that holds what Context.fluence_time gives for the flattened scene and the same seed"""
    scene = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
    defines = {"samples": "2", "tMin": "4", "tMax": "9", "tRes": "0.5", "medium": "homogeneous"}
    out = str(tmp_path / "phi.npy")
    args = [os.path.join(ROOT, "mitsubaer_amd", "mer_render"), "--fluence=8,8,8", "--time-resolved", "--seed", "3", "-o", out]
    for k, v in defines.items():
        args += ["-D", "%s=%s" % (k, v)]
    r = subprocess.run(args + [scene], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "paths %d " % (128 * 96 * 2) in r.stdout and "out of window " in r.stdout
    data = np.load(out)
    assert data.shape == (10, 8, 8, 8, 3) and data.dtype == np.float32
    d, spp = host.flatten_xml(scene, defines)
    assert spp == 2 and d.integrator == P.INTEGRATOR_PTRACER
    phi, info = ctx.fluence_time(d, (8, 8, 8), 10, d.min_bound, d.bin_width, spp, seed=3)
    assert info["paths"] == 128 * 96 * 2 and phi.sum() > 0 and (phi.sum((1, 2, 3, 4)) > 0).sum() >= 5
    printed = [float(v) for v in r.stdout.split("out of window ")[1].split()[:3]]
    np.testing.assert_allclose(printed, info["out_of_window"], rtol=1e-6)
    np.testing.assert_allclose(data, phi.astype(np.float32), rtol=1e-6, atol=0)
