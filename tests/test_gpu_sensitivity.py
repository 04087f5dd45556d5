"""The sensitivity grid of a detector on the boundary (mer_render_sensitivity, mer_sensitivity.hpp) on the GPU: two closed forms (the clear
cube's column, the pure absorber), the exitance map's walk and window sum, the accounting identity sum(sums) + dropped = w x path length,
the float64 restatement tests/sensitivity64.py per cell, the derivative of the detected signal by sigma_a on straight and curved rays, the
launch shapes of the two-pass loop, and the interface: accumulate / clear, the bounds-checking build, the refusals, `mer_render --sensitivity`.

Set-up: a 16 x 16 film (path enumeration only), the cube [-1, 1]^3 or the unit sphere, the beam of power (5, 3, 8) from (0.25, 0.25, -3)
along +z, grids of 4^3 or 8^3 cells, rasters of 4 x 4 cells per face: the beam leaves through raster cell (2, 2) of face 5 and runs along
the grid column ix = iy = 2 of a 4^3 grid."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host, volio
from tests import sensitivity64 as S
from tests import test_sensitivity64 as T
from tests import test_gpu_exitance as TE
from tests import test_gpu_lightpath_parent as TPAR
from tests import test_gpu_ptracer as TP

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 16
POWER3 = [float(v) for v in T.POWER3]
BEAM_O = [0.25, 0.25, -3.0]
CUBE = ((-1, -1, -1), (1, 1, 1))
RTOL_SUM = 1e-12         # float64 sums of the same terms in another order (the issue's bound)
RTOL_PIECE = 1e-5        # float32 arithmetic of the pieces


def _beam(o=BEAM_O):
    return P.collimated_emitter(TP._beam_frame(o, [0.0, 0.0, 1.0]), POWER3)


def _det(sc, face=5, window=(2, 3, 2, 3), res=(4, 4), **kw):
    return capi.detector_desc(sc.boundary, res, face, window, **kw)


def _render(ctx, p, det_kw, spp, res=(4, 4, 4), box=CUBE, seed=1, counters=False):
    """one sensitivity render: (raw sums, totals[, counters])"""
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.sensitivity_create(res, box[0], box[1], _det(sc, **det_kw))
    try:
        ctx.counters_reset()
        ctx.render_sensitivity(sc, h, 0, spp, seed=seed)
        cnt = [int(v) for v in ctx.counters()]
        s, t = ctx.sensitivity_read(h)
    finally:
        ctx.sensitivity_destroy(h)
        for v in vols:
            v.destroy()
    assert np.isfinite(s).all() and np.isfinite(t).all() and not t[13:].any()
    return (s, t, cnt) if counters else (s, t)


def _column(res=(4, 4, 4)):
    on = np.zeros((res[2], res[1], res[0]), bool); on[:, 2 * res[1] // 4, 2 * res[0] // 4] = True
    return on


# ---- 1. closed forms -------------------------------------------------------------------------------------------------------------------

def test_clear_cube_column(ctx):
    spp = 16
    paths = W * H * spp
    s, t = _render(ctx, TE._clear(emitters=[_beam()]), {}, spp)
    on = _column()
    assert np.all(s[~on] == 0.0)
    np.testing.assert_allclose(s[on], np.broadcast_to(paths * np.array(POWER3) * 0.5, (4, 3)), rtol=RTOL_PIECE, atol=0)
    assert t[0] == paths and t[8] == paths and t[12] == 0 and t[7] == 0 and not t[4:7].any()
    np.testing.assert_array_equal(t[1:4], paths * np.array(POWER3))
    np.testing.assert_allclose(t[9:12], paths * np.array(POWER3) * 2.0, rtol=RTOL_PIECE, atol=0)
    # the window on the entry face: nothing is detected, nothing is replayed, no error
    s0, t0 = _render(ctx, TE._clear(emitters=[_beam()]), dict(face=4, window=(0, 4, 0, 4)), spp)
    assert not s0.any() and t0[0] == paths and not t0[1:].any()


def test_pure_absorber_column(ctx):
    """sigma_s = 0: the detected paths are those whose first flight passes the cube, each with w = P: J_c = detected P 2 / nz exactly given
    the count, which is binomial with p = exp(-2 sigma_t)"""
    spp, k = 64, 4
    paths = W * H * spp
    counts = []
    for j in range(k):
        s, t = _render(ctx, TE._absorber(emitters=[_beam()]), {}, spp, seed=40 + j)
        on = _column()
        assert np.all(s[~on] == 0.0) and t[12] == 0 and t[0] == paths
        np.testing.assert_allclose(s[on], np.broadcast_to(t[8] * np.array(POWER3) * 0.5, (4, 3)), rtol=RTOL_PIECE, atol=0)
        np.testing.assert_array_equal(t[1:4], t[8] * np.array(POWER3))
        counts.append(t[8])
    p = np.exp(-2 * TE.T.ABSORBER)
    z = abs(sum(counts) - k * paths * p) / np.sqrt(k * paths * p * (1 - p))
    print("detected %d of %d, expected %.1f, z %.2f" % (sum(counts), k * paths, k * paths * p, z))
    assert z <= 4 and min(counts) > 64


# ---- 2. the exitance map's walk --------------------------------------------------------------------------------------------------------

_RGB = dict(sigma_s=[1.0, 0.8, 1.3], sigma_a=[0.2, 0.3, 0.1])
WALKS = {
    "straight homogeneous RGB": (lambda: TE._base(emitters=[_beam()], **_RGB), dict(face=5, window=(1, 4, 0, 3))),
    "straight homogeneous RGB sphere": (lambda: TE._base(emitters=[_beam()], **_RGB, **TE._sphere()), dict(face=0, window=(0, 3, 2, 4))),
    "straight gridded sigma_t": (lambda: TE._grid(emitters=[_beam()]), dict(face=5, window=(1, 4, 0, 3))),
    "trilinear Verlet": (lambda: TPAR.SCENES["trilinear_verlet"](), dict(face=5, window=(0, 4, 0, 4))),
    "trilinear RK4": (lambda: TPAR.SCENES["trilinear_rk4"](), dict(face=5, window=(0, 4, 0, 4))),
    "B-spline Verlet": (lambda: TPAR.SCENES["bspline"](), dict(face=5, window=(0, 4, 0, 4), t_bin=4.5)),      # n = 2 - (r / R)^2: the straight passage ends near 5.8
    "acoustic RK4": (lambda: TPAR.SCENES["acoustic"](), dict(face=5, window=(0, 4, 0, 4))),
}
CONE_GATE = dict(cos_min=0.3, t_min=2.0, t_bin=3.5)      # the exterior leg is 2; a straight passage through the cube ends at 4 ... 4.7


@pytest.mark.parametrize("which", list(WALKS))
def test_same_walk_and_window_sum_as_the_exitance_map(ctx, which):
    make, dk = WALKS[which]
    spp = 16
    p = make()
    gate = dict(CONE_GATE, t_bin=dk.get("t_bin", CONE_GATE["t_bin"]))
    s, t, cnt = _render(ctx, p, dict(dk, **gate), spp, res=(8, 8, 8), seed=7, counters=True)
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    he = ctx.exitance_create(sc.boundary, (4, 4), frames=1, **gate)
    try:
        ctx.counters_reset()
        ctx.render_exitance(sc, he, 0, spp, seed=7)
        cnt_e = [int(v) for v in ctx.counters()]
        m, te = ctx.exitance_read(he)
        exits = ctx.exitance(sc, (4, 4), spp, seed=7)[1][14]
    finally:
        ctx.exitance_destroy(he)
        for v in vols:
            v.destroy()
    iu0, iu1, iv0, iv1 = dk["window"]
    window = m[0, dk["face"], iv0:iv1, iu0:iu1].reshape(-1, 3).sum(0)
    print(which, "paths", t[0], "detected", t[8], "of", exits, "exits; W_det", t[1:4], "window", window, "late", te[8], "rejected", te[11])
    assert cnt == cnt_e and cnt[capi.C_PATHS] == W * H * spp
    assert t[0] == te[0] == W * H * spp and t[7] == te[7]
    np.testing.assert_allclose(t[1:4], window, rtol=RTOL_SUM, atol=0)
    assert t[12] == 0
    assert 0 < t[8] < exits and te[8] > 0 and te[11] > 0               # the cone and the gate reject some exits, not all
    assert s.sum() > 0


# ---- 3. the accounting identity --------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["straight homogeneous RGB", "straight homogeneous RGB sphere", "trilinear Verlet", "acoustic RK4",
                                   "straight gridded sigma_t", "trilinear RK4", "B-spline Verlet"])
def test_cells_and_dropped_hold_all_of_the_path_length(ctx, which):
    make, dk = WALKS[which]
    dk = {k: v for k, v in dk.items() if k != "t_bin"}                   # the width of the walk test's gate, which starts at CONE_GATE's t_min
    s, t = _render(ctx, make(), dk, 16, res=(5, 4, 3), box=((-0.6, -0.5, -0.7), (0.5, 0.7, 0.4)), seed=11)
    lhs = s.reshape(-1, 3).sum(0) + t[4:7]
    print(which, "cells + dropped", lhs, "w x length", t[9:12], "dropped", t[4:7])
    assert np.all(t[4:7] > 0) and t[8] > 64 and t[12] == 0
    np.testing.assert_allclose(lhs, t[9:12], rtol=RTOL_PIECE, atol=0)


# ---- 4. against the float64 restatement ------------------------------------------------------------------------------------------------

SCATTER = dict(sigma_s=np.array([1.0, 0.8, 1.3]), sigma_a=np.array([0.2, 0.3, 0.1]), g=0.5, window=(1, 3, 1, 3))
K = 16


def test_scattering_cube_matches_float64(ctx):
    """16 batches of 4096 paths; the library's default strategy (balance) on a chromatic sigma_t, medium_sampling_weight 1"""
    spp = 16
    ref, rt = S.render(T.BEAM, T.POWER3, S.LP.homogeneous(SCATTER["sigma_s"], SCATTER["sigma_a"], "balance"), SCATTER["g"], (4, 4, 4),
                       S.detector((4, 4), 5, SCATTER["window"]), paths=W * H * spp, batches=K, seed=21)
    p = TE._base(emitters=[_beam()], sigma_s=list(SCATTER["sigma_s"]), sigma_a=list(SCATTER["sigma_a"]), g=SCATTER["g"])
    got = [_render(ctx, p, dict(window=SCATTER["window"]), spp, seed=900 + j) for j in range(K)]
    s = np.array([g[0] for g in got]); t = np.array([g[1] for g in got])
    assert np.all(t[:, 0] == W * H * spp) and np.all(t[:, 12] == 0) and np.all(t[:, 7] == 0) and not t[:, 4:7].any()
    S.bar(s.mean(0), s.std(0, ddof=1) / np.sqrt(K), ref.mean(0), ref.var(0, ddof=1) / K, what="sensitivity cells")
    for c in range(3):
        for q, name in ((1, "detected weight"), (9, "weight x length")):
            S.total_bar(t[:, q + c], rt[:, q + c].mean(), rt[:, q + c].var(ddof=1) / K, what="%s, channel %d" % (name, c))
    S.total_bar(t[:, 8], rt[:, 8].mean(), rt[:, 8].var(ddof=1) / K, what="detected paths")


# ---- 5. the derivative of the detected signal ------------------------------------------------------------------------------------------

def _signal(ctx, p, dk, spp, seed):
    """the detected signal from mer_render_exitance: the sum of the window's cells of a one-frame map with the detector's cone"""
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    m, t = ctx.exitance(sc, (4, 4), spp, cos_min=dk.get("cos_min", 0.0), seed=seed)
    for v in vols:
        v.destroy()
    iu0, iu1, iv0, iv1 = dk["window"]
    return m[0, dk["face"], iv0:iv1, iu0:iu1].reshape(-1, 3).sum(0), t


@pytest.mark.parametrize("which", ["straight", "curved"])
def test_jacobian_is_minus_the_derivative_of_the_signal(ctx, which):
    """strategy manual at a fixed density, medium_sampling_weight set, the roulette out of reach, at most 20 flights: the walks at
    sigma_a +- delta are the same paths.  Straight: the central difference of the exitance signal equals -sum(J) to 2e-3 (the truncation
    delta^2 L^2 / 6, L < 70).  Curved (n = 1.3 + 0.15 y on 16^3 nodes, stepsize h): the last piece before the boundary deposits nothing, so
    sum(J) may fall short by at most 1.5 h / Lbar, Lbar = totals[9..11] / totals[1..3], and exceed by no more than 2e-3"""
    D = T.DERIV
    h, spp, seed = 0.05, 16, 5
    dk = dict(face=5, window=(1, 3, 1, 3), cos_min=0.2)
    curved = dict(rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=h, stepper=P.STEP_VERLET) if which == "curved" else {}

    def scene(shift):
        return TE._base(emitters=[_beam()], sigma_s=list(D["sigma_s"]), sigma_a=list(D["sigma_a"] + shift), g=D["g"], strategy=P.STRATEGY_MANUAL,
                        sampling_density=D["density"], medium_sampling_weight=D["weight"], rr_depth=D["rr_depth"], max_depth=D["max_depth"], **curved)
    s, t = _render(ctx, scene(0.0), dk, spp, seed=seed)
    wp, tp = _signal(ctx, scene(+D["delta"]), dk, spp, seed)
    wm, tm = _signal(ctx, scene(-D["delta"]), dk, spp, seed)
    w0, _ = _signal(ctx, scene(0.0), dk, spp, seed)
    assert tp[14] == tm[14] and tp[7] == tm[7] == t[7]                      # the same paths left
    np.testing.assert_allclose(t[1:4], w0, rtol=RTOL_SUM, atol=0)
    assert t[12] == 0 and 64 < t[8] < W * H * spp and not t[4:7].any()
    deriv = (wp - wm) / (2 * D["delta"])
    jsum = s.reshape(-1, 3).sum(0)
    ratio = jsum / -deriv
    lbar = t[9:12] / t[1:4]
    print(which, "dW/dsigma_a", deriv, "-sum(J)", -jsum, "sum(J) / -derivative", ratio, "Lbar", lbar)
    assert np.all(lbar < 70.0)
    if which == "straight":
        np.testing.assert_allclose(jsum, -deriv, rtol=T.DERIV_RTOL, atol=0)
    else:
        assert np.all(ratio >= 1.0 - 1.5 * h / lbar) and np.all(ratio <= 1.0 + T.DERIV_RTOL), (ratio, 1.5 * h / lbar)


# ---- 6. launch shapes ------------------------------------------------------------------------------------------------------------------

def test_partial_tiles_leave_lanes_without_a_path(ctx):
    """a 40 x 24 film: two tiles, 960 of 2048 work ids per sample inside the image"""
    spp = 3
    s, t = _render(ctx, TE._clear(emitters=[_beam()], w=40, h=24), {}, spp)
    paths = 40 * 24 * spp
    assert t[0] == paths and t[8] == paths and t[12] == 0
    on = _column()
    assert np.all(s[~on] == 0.0)
    np.testing.assert_allclose(s[on], np.broadcast_to(paths * np.array(POWER3) * 0.5, (4, 3)), rtol=RTOL_PIECE, atol=0)


def test_a_render_of_two_chunks_equals_its_half_shards(ctx):
    """a curved clear scene of 32 x 32 x 65 paths = 66 560: one more chunk than PT_PATHS_PER_LAUNCH_CURVED (65 536) holds"""
    p = TE._clear(rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=0.05, stepper=P.STEP_VERLET, emitters=[_beam()], w=32, h=32)
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.sensitivity_create((4, 4, 4), *CUBE, _det(sc, window=(0, 4, 0, 4)))
    try:
        ctx.render_sensitivity(sc, h, 0, 65, seed=2)
        whole, tw = ctx.sensitivity_read(h)
        parts = []
        for begin, count in ((0, 32), (32, 33)):
            ctx.sensitivity_clear(h)
            z, tz = ctx.sensitivity_read(h)
            assert not z.any() and not tz.any()
            ctx.render_sensitivity(sc, h, begin, count, seed=2)
            parts.append(ctx.sensitivity_read(h))
        assert tw[0] == tw[8] == 32 * 32 * 65 > 65536 and tw[12] == 0 and whole.sum() > 0
        assert parts[0][1][0] == 32 * 32 * 32 and parts[1][1][0] == 32 * 32 * 33
        np.testing.assert_allclose(parts[0][0] + parts[1][0], whole, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(parts[0][1] + parts[1][1], tw, rtol=RTOL_SUM, atol=0)
        # the grid accumulates: the first half on top of the second
        ctx.render_sensitivity(sc, h, 0, 32, seed=2)
        both, tb = ctx.sensitivity_read(h)
        np.testing.assert_allclose(both, whole, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(tb, tw, rtol=RTOL_SUM, atol=0)
        _, t_only = ctx.sensitivity_read(h, sums=False)
        assert np.array_equal(t_only, tb)
    finally:
        ctx.sensitivity_destroy(h)
        for v in vols:
            v.destroy()
    # the convenience call: J / paths and the totals by name
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    j, info = ctx.sensitivity(sc, (4, 4, 4), dict(res=(4, 4), face=5), 65, seed=2)
    np.testing.assert_allclose(j, whole / tw[0], rtol=RTOL_SUM, atol=0)
    assert info["paths"] == tw[0] and info["detected"] == tw[8] and info["disagreements"] == 0
    for v in vols:
        v.destroy()


@pytest.mark.parametrize("w,h,spp,want", [(1, 1, 1, 1), (16, 16, 1, 256)])
def test_detected_counts_of_one_and_of_several_waves(ctx, w, h, spp, want):
    """one chunk whose list holds a single record (one lane of the replay launch has a path) and one that holds four waves of them;
    a list of 0 records is test_clear_cube_column's entry-face window"""
    s, t = _render(ctx, TE._clear(emitters=[_beam()], w=w, h=h), {}, spp)
    assert t[0] == want and t[8] == want and t[12] == 0
    on = _column()
    assert np.all(s[~on] == 0.0)
    np.testing.assert_allclose(s[on], np.broadcast_to(want * np.array(POWER3) * 0.5, (4, 3)), rtol=RTOL_PIECE, atol=0)


# ---- 7. the bounds-checking build, the refusals, the command line ----------------------------------------------------------------------

def test_bounds_checking_build_agrees(ctx):
    cases = [WALKS[k] for k in ("straight gridded sigma_t", "trilinear Verlet", "straight homogeneous RGB sphere")]
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for make, dk in cases:
            got = [_render(cx, make(), dict(CONE_GATE, **dk), 16, res=(5, 3, 4), box=((-0.8, -0.9, -1.0), (0.9, 1.0, 0.7)), seed=3) for cx in (c, ctx)]
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (n, kind, idx, lim)
            assert got[0][0].sum() > 0 and got[0][1][8] > 0 and got[0][1][12] == 0
            np.testing.assert_allclose(got[0][0], got[1][0], rtol=RTOL_SUM, atol=0)
            np.testing.assert_allclose(got[0][1], got[1][1], rtol=RTOL_SUM, atol=0)
    finally:
        c.close()


def test_library_refusals(ctx):
    """mer_render_sensitivity's own checks (the Python front end's are bypassed by editing the flat scene); nothing is launched"""
    def desc(**kw):
        return ctx.upload_scene(TE._base(**kw))[0]
    h = ctx.sensitivity_create((4, 4, 4), *CUBE, _det(desc()))
    hf = ctx.fluence_create((4, 4, 4), *CUBE)
    he = ctx.exitance_create(P.BOUNDARY_AABB, (4, 4))

    def refused(sc, msg, handle=None):
        with pytest.raises(capi.MerError, match=msg):
            ctx.render_sensitivity(sc, h if handle is None else handle, 0, 1)
    try:
        sc = desc(); sc.integrator = P.INTEGRATOR_VOLPATH
        refused(sc, "mer_render_sensitivity: the scene's integrator must be ptracer")
        refused(desc(**TE._sphere()), "the scene's boundary differs from the detector's")
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
        sc = desc(); sc.n_emitters = 0
        refused(sc, "no emitter")
        # handles: the three kinds do not mix
        for other in (hf, he, h + 1000):
            refused(desc(), "mer_render_sensitivity: unknown sensitivity handle", handle=other)
        with pytest.raises(capi.MerError, match="mer_render_fluence: unknown fluence handle"):
            ctx.render_fluence(desc(), h, 0, 1)
        with pytest.raises(capi.MerError, match="mer_render_exitance: unknown exitance handle"):
            ctx.render_exitance(desc(), h, 0, 1)
        for call, handle, msg in ((ctx.sensitivity_clear, hf, "unknown sensitivity handle"), (ctx.sensitivity_destroy, he, "unknown sensitivity handle"),
                                  (ctx.fluence_clear, h, "unknown fluence handle"), (ctx.exitance_destroy, h, "unknown exitance handle"),
                                  (ctx.sensitivity_clear, h + 1000, "unknown sensitivity handle")):
            with pytest.raises(capi.MerError, match=msg):
                call(handle)
        t16 = np.zeros(16)
        for bad in (hf, he, 0, h + 1000):
            assert ctx.lib.mer_sensitivity_read(ctx.h, C.c_int32(bad), None, t16.ctypes.data_as(C.c_void_p)) != 0
            assert "unknown sensitivity handle" in ctx.lib.mer_last_error(ctx.h).decode()
        assert ctx.lib.mer_exitance_read(ctx.h, C.c_int32(h), None, t16.ctypes.data_as(C.c_void_p)) != 0
        assert "unknown exitance handle" in ctx.lib.mer_last_error(ctx.h).decode()
        # nothing was launched: the grid and its totals are still zero
        s, t = ctx.sensitivity_read(h)
        assert not s.any() and not t.any()
        # descs, past the Python check
        for kw, msg in ((dict(res=(0, 4, 4)), "res must lie in 1 ... 1024"), (dict(bmin=(1, -1, -1)), "bmin must be below bmax"),
                        (dict(boundary=P.BOUNDARY_SDF), "boundary must be the cube"), (dict(dres=(4, 5000)), "detector res must lie in 1 ... 4096"),
                        (dict(t_bin=-1.0), "t_bin must be finite and at least 0"), (dict(t_min=float("nan")), "t_min must be finite"),
                        (dict(cos_min=1.0), "cos_min must lie in"), (dict(reserved=1), "reserved must be 0"), (dict(face=6), "face must be one of"),
                        (dict(boundary=P.BOUNDARY_SPHERE, face=1), "face must be one of"), (dict(window=(0, 5, 0, 4)), "the window must lie inside the raster"),
                        (dict(window=(2, 2, 0, 4)), "the window is empty")):
            kw = dict(kw); reserved = kw.pop("reserved", 0)
            det = capi.detector_desc(kw.pop("boundary", P.BOUNDARY_AABB), kw.pop("dres", (4, 4)), kw.pop("face", 5), kw.pop("window", (0, 4, 0, 4)),
                                     kw.pop("cos_min", 0.0), kw.pop("t_min", 0.0), kw.pop("t_bin", 0.0))
            det.reserved = reserved
            d = capi.sensitivity_desc(kw.pop("res", (4, 4, 4)), kw.pop("bmin", (-1, -1, -1)), kw.pop("bmax", (1, 1, 1)), det)
            assert not kw
            out = C.c_int32(-1)
            assert ctx.lib.mer_sensitivity_create(ctx.h, C.byref(d), C.byref(out)) != 0 and out.value == 0
            err = ctx.lib.mer_last_error(ctx.h).decode()
            assert err.startswith("mer_sensitivity_create: ") and re.search(msg, err), err
            with pytest.raises(capi.MerError, match=msg):                      # the Python check gives the library's message
                capi.validate_sensitivity(d)
    finally:
        ctx.sensitivity_destroy(h); ctx.fluence_destroy(hf); ctx.exitance_destroy(he)


def test_mer_render_sensitivity_writes_the_python_calls_map(ctx, tmp_path):
    """mer_render --sensitivity=8,8,8 --detector=... on scenes/cfg_laser_clear.xml: the VOL of J / paths that Context.sensitivity gives"""
    scene = os.path.join(ROOT, "scenes", "cfg_laser_clear.xml")
    defines = {"samples": "1", "sigmaS": "0.8", "sigmaA": "0.05"}
    out = str(tmp_path / "j.vol")
    d, spp = host.flatten_xml(scene, defines)
    # the face most of the light leaves through
    m, te = ctx.exitance(d, (4, 4), spp, seed=3)
    face = int(np.argmax(m[0].sum((1, 2, 3))))
    args = [os.path.join(ROOT, "mitsubaer_amd", "mer_render"), "--sensitivity=8,8,8", "--detector=%d,4,4,0,4,1,3" % face, "--accept-cos=0.25", "--gate=0,50",
            "--seed", "3", "-o", out]
    for k, v in defines.items():
        args += ["-D", "%s=%s" % (k, v)]
    r = subprocess.run(args + [scene], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "paths %d " % (128 * 96) in r.stdout and "disagreements 0" in r.stdout
    data, lo, hi = volio.read_vol(out, mmap=False)
    assert data.shape == (8, 8, 8, 3) and data.dtype == np.float32
    j, info = ctx.sensitivity(d, (8, 8, 8), dict(res=(4, 4), face=face, window=(0, 4, 1, 3), cos_min=0.25, t_min=0.0, t_bin=50.0), spp, seed=3)
    assert info["paths"] == 128 * 96 and info["detected"] > 0 and j.sum() > 0
    np.testing.assert_allclose(data, j.astype(np.float32), rtol=1e-6, atol=0)
    got = [float(v) for v in re.search(r"detected weight (\S+) (\S+) (\S+)", r.stdout).groups()]
    np.testing.assert_allclose(got, info["detected_weight"], rtol=1e-6)
