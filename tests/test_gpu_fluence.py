"""The fluence grid recorded from light paths (mer_render_fluence, mer_fluence.hpp) on the GPU: against the closed forms a fluence grid must
obey (Beer-Lambert along an unscattered beam, exact zeros off the beam, the energy balance), against the float64 restatement
tests/fluence64.py per cell, against the light tracer's own walk (counters), along curved rays against a float64 RK4 trace of the beam, and
the interface: shards, clear / accumulate, the bounds-checking build, the refusals, `mer_render --fluence`.

Set-up (tests/test_fluence64.py): a 16 x 16 film (path enumeration only) x 64 samples = 16 384 paths per batch, K = 16 batches with seeds
s0 + j, the cube [-1, 1]^3, the beam of power 5 from (0.2, 0.1, -3) along +z, an 8 x 8 x 8 grid over the cube unless said otherwise.
medium_sampling_weight = 1 throughout: every free flight is drawn from the medium, so that the escaped weight is the power that leaves
(include/mer.h).  Statistics: the project's bar -- at most 1 + 1 % of the cells beyond 4 sigma, totals within 4 sigma."""
import functools
import os
import subprocess
import ctypes as C
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host, volio
from tests import scenes
from tests import fluence64 as F
from tests import test_fluence64 as T
from tests import test_gpu_ptracer as TP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 16
SPP = 64
K = T.K
PATHS = W * H * SPP
assert PATHS == T.PATHS
CAM = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
BEAM_O, BEAM_D = [0.2, 0.1, -3.0], [0.0, 0.0, 1.0]
CUBE = ((-1, -1, -1), (1, 1, 1))
RTOL_SUM = 1e-9          # one set of deposits added in two orders: at most 2^20 float64 adds per cell, each within 2^-53: 2^-33 = 1.2e-10, rounded up


def _base(**kw):
    base = dict(w=W, h=H, fov_x_deg=40.0, cam_to_world=CAM, phase=P.PHASE_HG, g=T.G, sigma_s=[T.SIGMA_S] * 3, sigma_a=[T.SIGMA_A] * 3,
                env_radiance=[0, 0, 0], rfilter=P.FILTER_BOX, rfilter_param=0.5, integrator=P.INTEGRATOR_PTRACER, medium_sampling_weight=1.0,
                rr_depth=5, emitters=[P.collimated_emitter(TP._beam_frame(BEAM_O, BEAM_D), [T.POWER] * 3)])
    base.update(kw)
    return scenes.homogeneous_scene(**base)


def _absorber(**kw):
    return _base(sigma_s=[0.0] * 3, sigma_a=[T.ABSORBER] * 3, g=0.0, **kw)


def _batches(ctx, p, seed0, res=T.RES, box=CUBE, k=K, layout=capi.LAYOUT_DENSE):
    """k batches with seeds seed0 + j into one grid, cleared in between: raw sums (k, nz, ny, nx, 3), totals (k, 8)"""
    sc, vols = ctx.upload_scene(p, layout=layout)
    h = ctx.fluence_create(res, box[0], box[1])
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


def _grey(sums):
    """a grey scene: the three channels hold the same sums (their atomics add in their own order); returns channel 0"""
    np.testing.assert_allclose(sums[..., 1], sums[..., 0], rtol=RTOL_SUM, atol=0)
    np.testing.assert_allclose(sums[..., 2], sums[..., 0], rtol=RTOL_SUM, atol=0)
    return sums[..., 0]


@functools.lru_cache(maxsize=None)
def _ref(which):
    """the float64 references, computed once"""
    if which == "cube":
        return F.render(T.BEAM, T.SIGMA_S, T.SIGMA_A, T.G, T.RES, paths=PATHS, batches=K, seed=11, rr_depth=5)
    return F.render(T.BEAM, T.SIGMA_S, T.SIGMA_A, T.G, paths=PATHS, batches=K, seed=12, rr_depth=5, **T.CUT)


def _against_ref(sums, tot, ref, what):
    r, rt = ref
    g = _grey(sums)
    F.bar(g.mean(0), g.std(0, ddof=1) / np.sqrt(K), r.mean(0), r.var(0, ddof=1) / K, what=what + " cells")
    F.total_bar(tot[:, 1], rt[:, 1].mean(), rt[:, 1].var(ddof=1) / K, what=what + " escaped")
    if rt[:, 4].any():
        F.total_bar(tot[:, 4], rt[:, 4].mean(), rt[:, 4].var(ddof=1) / K, what=what + " dropped")
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 7] == 0)          # no zero-length flight with these seeds (test_curved_scattering_balances)
    bal = T.SIGMA_A * (g.sum((1, 2, 3)) + tot[:, 4]) + tot[:, 1]
    F.total_bar(bal, PATHS * T.POWER, what=what + " balance")


# ---- 1. closed forms -------------------------------------------------------------------------------------------------------------------

def test_pure_absorber_is_beer_lambert(ctx):
    """first collisions only: the beam's column against P / sigma_t (e^{-sigma_t a_k} - e^{-sigma_t b_k}) under the binomial variance, every other
    cell exactly 0.0, and every path either deposits P / sigma_t once or escapes with P"""
    sums, tot = _batches(ctx, _absorber(), 100)
    g = _grey(sums)
    T.column_check(g, T.ABSORBER, PATHS, "absorber column")
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:] == 0)
    F.total_bar(tot[:, 1], PATHS * T.POWER * np.exp(-2 * T.ABSORBER), what="absorber escaped")
    np.testing.assert_allclose(T.ABSORBER * g.sum((1, 2, 3)) + tot[:, 1], PATHS * T.POWER, rtol=1e-6)      # a deposit is P tau / pdf in float32: four roundings of 6e-8


def test_max_depth_2_is_the_ballistic_fluence(ctx):
    sums, tot = _batches(ctx, _base(max_depth=2), 200)
    T.column_check(_grey(sums), T.SIGMA_S + T.SIGMA_A, PATHS, "ballistic column")
    assert np.all(tot[:, 7] == 0)


# ---- 2., 3. against the float64 restatement --------------------------------------------------------------------------------------------

def test_scattering_medium_matches_float64(ctx):
    sums, tot = _batches(ctx, _base(), 300)
    _against_ref(sums, tot, _ref("cube"), "cube")


def test_box_that_cuts_the_shape_matches_float64(ctx):
    """a 4 x 6 x 5 grid over (-1, -0.5, -1) ... (0.5, 1, 0.25): a transposed or off-by-one index cannot pass"""
    sums, tot = _batches(ctx, _base(), 400, res=T.CUT["res"], box=(T.CUT["bmin"], T.CUT["bmax"]))
    assert sums.shape == (K, 5, 6, 4, 3)
    assert np.all(tot[:, 4] > 0)
    _against_ref(sums, tot, _ref("cut"), "cut")


# ---- 4. the light tracer's walk --------------------------------------------------------------------------------------------------------

def test_same_walk_as_the_light_tracer(ctx):
    """homogeneous straight scene: the light tracer's connections draw no sampler numbers there, so the two kernels walk the same paths:
    the same path, segment and real-collision counts, exactly"""
    sc, _ = ctx.upload_scene(_base())
    ctx.counters_reset()
    ctx.render_to_host(sc, 0, SPP, seed=7)
    a = ctx.counters()
    ctx.counters_reset()
    h = ctx.fluence_create(T.RES, *CUBE)
    try:
        ctx.render_fluence(sc, h, 0, SPP, seed=7)
        b = ctx.counters()
    finally:
        ctx.fluence_destroy(h)
    print("light tracer", a[:8], "fluence", b[:8])
    assert a[capi.C_PATHS] == PATHS and a[capi.C_REAL] > PATHS
    for c in (capi.C_PATHS, capi.C_SEGMENTS, capi.C_REAL):
        assert a[c] == b[c], (c, a[c], b[c])


# ---- 5. gridded sigma_t ----------------------------------------------------------------------------------------------------------------

def test_gridded_sigma_matches_homogeneous(ctx):
    """a constant 16^3 density with scale = sigma_t (delta tracking, deposits 1 / sigma_t) against the homogeneous medium (the exponential
    strategy, deposits tau / pdf): per cell within the bar, with both batch spreads"""
    st = T.SIGMA_S + T.SIGMA_A
    grid = _base(sigma_mode=P.SIGMA_GRID, density=np.ones((16, 16, 16), np.float32), density_scale=st, albedo=[T.SIGMA_S / st] * 3)
    a, ta = _batches(ctx, grid, 500)
    b, tb = _batches(ctx, _base(), 600)
    ga, gb = _grey(a), _grey(b)
    F.bar(ga.mean(0), ga.std(0, ddof=1) / np.sqrt(K), gb.mean(0), gb.var(0, ddof=1) / K, what="grid vs homogeneous")
    F.total_bar(ta[:, 1], tb[:, 1].mean(), tb[:, 1].var(ddof=1) / K, what="grid escaped")
    F.total_bar(T.SIGMA_A * ga.sum((1, 2, 3)) + ta[:, 1], PATHS * T.POWER, what="grid balance")
    assert np.all(ta[:, 7] == 0)


# ---- 6. curved paths -------------------------------------------------------------------------------------------------------------------

def _rif():
    yy = np.linspace(-1, 1, 5)
    return np.broadcast_to((TP.RIF_A + TP.RIF_B * yy)[None, :, None], (5, 5, 5)).astype(np.float32).copy()


@functools.lru_cache(maxsize=None)
def _beam_trace(h=0.002):
    """the beam through n = RIF_A + RIF_B y in float64 (RK4 of dp/ds = v / n, dv/ds = grad n: s is the arc length): points (n, 3) at arc
    lengths s (n,), from the entry face z = -1 to the exit of the cube; the last step is shortened by bisection"""
    p = np.array([BEAM_O[0], BEAM_O[1], -1.0]); v = np.array(BEAM_D) * (TP.RIF_A + TP.RIF_B * p[1])
    pts, ss, s = [p.copy()], [0.0], 0.0
    for _ in range(100000):
        q, w = TP._rk4(p, v, h)
        if np.all(np.abs(q) <= 1):
            p, v, s = q, w, s + h
            pts.append(p.copy()); ss.append(s)
            continue
        lo, hi = 0.0, h
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            q, _w = TP._rk4(p, v, mid)
            if np.all(np.abs(q) <= 1):
                lo = mid
            else:
                hi = mid
        q, _w = TP._rk4(p, v, lo)
        pts.append(q); ss.append(s + lo)
        return np.array(pts), np.array(ss)
    raise AssertionError("the beam never left the cube")


@pytest.mark.parametrize("stepper", [P.STEP_VERLET, P.STEP_RK4])
def test_curved_beam_follows_the_float64_trace(ctx, stepper):
    """n = 1.3 + 0.15 y on a 5^3 dense grid, stepsize 0.05, a pure absorber: per z slab the centroid of the deposits (cell centres weighted by
    the sums) lies within half a cell of the beam's deposit-weighted mean position in that slab, and the deposited fraction is
    1 - e^{-sigma_t L} with L the traced arc length to the exit (binomial variance)"""
    pts, s = _beam_trace()
    L = s[-1]
    assert pts[-1][2] > 1 - 1e-9 and pts[:, 1].max() - pts[:, 1].min() > 0.15           # leaves through z = 1, having bent by more than half a cell
    sums, tot = _batches(ctx, _absorber(rif_mode=P.RIF_TRILINEAR, rif=_rif(), stepsize=0.05, stepper=stepper), 700 + stepper)
    g = _grey(sums).sum(0)                                                            # (nz, ny, nx)
    centres = -1 + (np.arange(8) + 0.5) * 0.25
    wgt = np.exp(-T.ABSORBER * s)
    worst = 0.0
    for kz in range(8):
        slab = g[kz]
        assert slab.sum() > 0
        cy = (slab.sum(1) * centres).sum() / slab.sum(); cx = (slab.sum(0) * centres).sum() / slab.sum()
        m = (pts[:, 2] >= -1 + 0.25 * kz) & (pts[:, 2] < -1 + 0.25 * (kz + 1))
        by = np.average(pts[m, 1], weights=wgt[m]); bx = np.average(pts[m, 0], weights=wgt[m])
        worst = max(worst, abs(cy - by), abs(cx - bx))
    print("stepper %d: arc length %.5f, largest centroid offset %.4f (half a cell: 0.125)" % (stepper, L, worst))
    assert worst <= 0.125
    pdep = 1 - np.exp(-T.ABSORBER * L)
    frac = T.ABSORBER * _grey(sums).sum() / (K * PATHS * T.POWER)
    z = abs(frac - pdep) / np.sqrt(pdep * (1 - pdep) / (K * PATHS))
    print("deposited fraction %.6f, 1 - exp(-sigma_t L) = %.6f, z %.2f" % (frac, pdep, z))
    assert z <= 4
    assert np.all(tot[:, 4:] == 0)


@pytest.mark.parametrize("stepper", [P.STEP_VERLET, P.STEP_RK4])
def test_curved_scattering_balances(ctx, stepper):
    """sigma_a > 0 and scattering along curved rays: absorbed + escaped = emitted, and no path ended by a budget.
    The seeds: a sampler value of exactly 0 (probability 2^-23 per free flight, 1.2e6 free flights here: 0.15 expected) is a flight of length
    0, which the walk -- the light tracer's -- ends as "no forward progress" and totals[7] counts.  Paths are a function of the seed alone, and
    with these seeds none occurs (measured: base 800 and 1300 hold one such path each, 1000, 1100 and 1200 none, with either stepper)."""
    sums, tot = _batches(ctx, _base(rif_mode=P.RIF_TRILINEAR, rif=_rif(), stepsize=0.05, stepper=stepper), 1000 + stepper)
    assert np.all(tot[:, 7] == 0) and np.all(tot[:, 4:7] == 0)
    F.total_bar(T.SIGMA_A * _grey(sums).sum((1, 2, 3)) + tot[:, 1], PATHS * T.POWER, what="curved balance")


# ---- 7. shards, clear, accumulate ------------------------------------------------------------------------------------------------------

def test_half_shards_add_up_and_the_grid_accumulates(ctx):
    sc, _ = ctx.upload_scene(_base())
    h = ctx.fluence_create(T.RES, *CUBE)
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
        # the second half went into a cleared grid; the first half on top of it accumulates to the whole
        ctx.render_fluence(sc, h, 0, 32, seed=9)
        both, tb = ctx.fluence_read(h)
        np.testing.assert_allclose(both, whole, rtol=RTOL_SUM, atol=0)
        assert tb[0] == PATHS
        _, t_only = ctx.fluence_read(h, sums=False)
        assert np.array_equal(t_only, tb)
    finally:
        ctx.fluence_destroy(h)


# ---- 8. the bounds-checking build ------------------------------------------------------------------------------------------------------

def test_bounds_checking_build_agrees(ctx):
    """libmer_check.so: a straight gridded scene and a curved scene form no index outside a device buffer (the cell index goes through the
    check), and give the product build's grids"""
    st = T.SIGMA_S + T.SIGMA_A
    cases = (_base(sigma_mode=P.SIGMA_GRID, density=np.ones((16, 16, 16), np.float32), density_scale=st, albedo=[T.SIGMA_S / st] * 3),
             _base(rif_mode=P.RIF_TRILINEAR, rif=_rif(), stepsize=0.05, stepper=P.STEP_VERLET))
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for p in cases:
            got = []
            for cx in (c, ctx):
                sc, vols = cx.upload_scene(p, layout=capi.LAYOUT_DENSE)
                phi, info = cx.fluence(sc, T.CUT["res"], SPP, seed=3, bmin=T.CUT["bmin"], bmax=T.CUT["bmax"])
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


# ---- 9. refusals -----------------------------------------------------------------------------------------------------------------------

def test_library_refusals(ctx):
    """mer_render_fluence's own checks (the Python front end's are bypassed by editing the flat scene)"""
    h = ctx.fluence_create(T.RES, *CUBE)

    def desc(**kw):
        return ctx.upload_scene(_base(**kw))[0]

    def refused(sc, msg, handle=None):
        with pytest.raises(capi.MerError, match=msg):
            ctx.render_fluence(sc, h if handle is None else handle, 0, 1)
    try:
        sc = desc(); sc.integrator = P.INTEGRATOR_VOLPATH
        refused(sc, "integrator must be ptracer")
        sc = desc(); sc.sensor = P.SENSOR_ORTHOGRAPHIC
        refused(sc, "perspective sensor only")
        sc = desc(); sc.boundary_bsdf = P.BSDF_HDIELECTRIC
        refused(sc, "dielectric boundaries")
        sc = desc(); sc.boundary = P.BOUNDARY_SDF
        refused(sc, "signed-distance")
        sc = desc(); sc.emitters[0].type = P.EMITTER_AREA
        refused(sc, "area emitters")
        sc = desc(); sc.emitters[0].type = P.EMITTER_ENVMAP
        refused(sc, "envmap")
        sc = desc(); sc.env_radiance[1] = 0.5
        refused(sc, "env_radiance")
        sc = desc(); sc.n_emitters = 0
        refused(sc, "no emitter")
        sc, vols = ctx.upload_scene(_base(rif_mode=P.RIF_TRILINEAR, rif=np.ones((6, 6, 6), np.float32), stepsize=0.05), layout=capi.LAYOUT_CELL8)
        refused(sc, "dense layout")
        for v in vols:
            v.destroy()
        # nothing was launched: the grid is still zero
        s, t = ctx.fluence_read(h)
        assert not s.any() and not t.any()
        # handles
        refused(desc(), "unknown fluence handle", handle=h + 1000)
        for call in (ctx.fluence_clear, ctx.fluence_destroy):
            with pytest.raises(capi.MerError, match="unknown fluence handle"):
                call(h + 1000)
        with pytest.raises(capi.MerError, match="unknown fluence handle"):
            ctx.fluence_read(h + 1000)
        t8 = np.zeros(8)
        assert ctx.lib.mer_fluence_read(ctx.h, C.c_int32(0), None, t8.ctypes.data_as(C.c_void_p)) != 0
        # descs, past the Python check
        for res, lo, hi, msg in (((0, 8, 8), (-1, -1, -1), (1, 1, 1), "res must lie in 1 ... 1024"), ((8, 8, 2000), (-1, -1, -1), (1, 1, 1), "res must lie in 1 ... 1024"),
                                 ((1024, 1024, 129), (-1, -1, -1), (1, 1, 1), "2\\^27 cells"), ((8, 8, 8), (-1, 1, -1), (1, 1, 1), "bmin must be below bmax"),
                                 ((8, 8, 8), (-1, -1, -1), (1, float("nan"), 1), "finite")):
            d = capi.fluence_desc(res, lo, hi); out = C.c_int32(-1)
            assert ctx.lib.mer_fluence_create(ctx.h, C.byref(d), C.byref(out)) != 0 and out.value == 0
            assert __import__("re").search(msg, ctx.lib.mer_last_error(ctx.h).decode())
    finally:
        ctx.fluence_destroy(h)


# ---- 10. the command line --------------------------------------------------------------------------------------------------------------

def test_mer_render_fluence_writes_the_python_calls_grid(ctx, tmp_path):
    """mer_render --fluence=8,8,8 on the laser example: a 3-channel float32 VOL over the box of the cell centres that holds the grid
    Context.fluence gives for the same scene and seed"""
    scene = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
    defines = {"samples": "2", "tMin": "4", "tMax": "9", "tRes": "0.5", "medium": "homogeneous"}
    out = str(tmp_path / "phi.vol")
    args = [os.path.join(ROOT, "mitsubaer_amd", "mer_render"), "--fluence=8,8,8", "--seed", "3", "-o", out]
    for k, v in defines.items():
        args += ["-D", "%s=%s" % (k, v)]
    r = subprocess.run(args + [scene], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "paths %d " % (128 * 96 * 2) in r.stdout and "ended 0" in r.stdout
    data, lo, hi = volio.read_vol(out, mmap=False)
    assert data.shape == (8, 8, 8, 3) and data.dtype == np.float32
    np.testing.assert_allclose(lo, [-0.875] * 3, rtol=0, atol=1e-7); np.testing.assert_allclose(hi, [0.875] * 3, rtol=0, atol=1e-7)
    d, spp = host.flatten_xml(scene, defines)
    assert spp == 2 and d.integrator == P.INTEGRATOR_PTRACER
    phi, info = ctx.fluence(d, (8, 8, 8), spp, seed=3)
    assert info["paths"] == 128 * 96 * 2 and phi.sum() > 0
    assert not np.allclose(phi[..., 0], phi[..., 2])                       # a chromatic medium: the channels differ
    np.testing.assert_allclose(data, phi.astype(np.float32), rtol=1e-6, atol=0)
