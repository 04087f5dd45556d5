"""Detector arrays, gates and the scattering grid of the sensitivity map (mer_sensitivity_array_create, mer_sensitivity.hpp) on the GPU:
the single-detector entry point as the exact reference of every measurement's J, the sums that tie the measurements to the totals, closed
forms of K (nothing scatters; every path detected: the collision fluence grid), the float64 restatement tests/sensitivity_array64.py per
cell, the derivative of the detected signal by sigma_s on straight and curved rays, the launch shapes, the bounds-checking build, the
refusals and `mer_render --detector-bins --gates --scatter`.

Set-up: test_gpu_sensitivity.py's -- a 16 x 16 film (path enumeration only), the cube [-1, 1]^3 or the unit sphere, the beam of power
(5, 3, 8) from (0.25, 0.25, -3) along +z, grids of 4^3 ... 8^3 cells, rasters of 4 x 4 cells per face."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host
from tests import test_sensitivity_array64 as TA
from tests import test_gpu_exitance as TE
from tests import test_gpu_sensitivity as TS
from tests import test_gpu_sensitivity_media as TM
from tests.test_gpu_sensitivity import WALKS, _beam, RTOL_SUM, RTOL_PIECE
from tests.test_sensitivity64 import DERIV, DERIV_RTOL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W = H = 16
CUBE = TS.CUBE
RAGGED = ((5, 4, 3), ((-0.6, -0.5, -0.7), (0.5, 0.7, 0.4)))
POWER3 = np.array(TS.POWER3)


def _array(ctx, p, det_kw, bins, gates, scatter, spp, res=(4, 4, 4), box=CUBE, seed=1, begin=0):
    """one array render: (raw sums [1 + scatter][gates][ndv][ndu][nz][ny][nx][3], meas, totals)"""
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.sensitivity_array_create(res, box[0], box[1], TS._det(sc, **det_kw), bins, gates, scatter)
    try:
        ctx.render_sensitivity(sc, h, begin, spp, seed=seed)
        s, m, t = ctx.sensitivity_read_array(h)
        assert ctx.sensitivity_shape(h) == s.shape[1:4] + (int(scatter),)
    finally:
        ctx.sensitivity_destroy(h)
        for v in vols:
            v.destroy()
    assert np.isfinite(s).all() and np.isfinite(m).all() and np.isfinite(t).all() and not m[..., 7].any()
    if not scatter:
        assert not t[13:].any() and not m[..., 4:7].any()
    return s, m, t


# ---- 1. the partition identity: the single-detector entry point is the reference ------------------------------------------------------------

# the first gate of each walk: four gates of width 0.5 (a power of two, t_min a multiple of it: l - t_min and the division are exact in
# float32, so the array's gate g and the single detector's gate (t_min + g t_bin, t_bin) cannot disagree at an edge).  The exterior leg is 2;
# a straight passage ends at 4 ... 4.7 in the cube, from 3 on in the sphere, at 4.6 ... in n = 1.3 + 0.15 y and the acoustic field, near
# 5.8 in the B-spline field
T_MIN = {"straight homogeneous RGB": 4.0, "straight homogeneous RGB sphere": 3.0, "straight gridded sigma_t": 4.0, "trilinear Verlet": 4.5,
         "trilinear RK4": 4.5, "B-spline Verlet": 5.5, "acoustic RK4": 4.5}
T_BIN, GATES = 0.5, 4


@pytest.mark.parametrize("which", list(WALKS))
def test_every_measurement_is_the_single_detector_render(ctx, which):
    """a 4 x 4 raster, the whole face in 2 x 2 bins, 4 gates, the cone 0.3, 16 spp: slice m of J is the grid of mer_sensitivity_create with
    m's sub-window and gate, meas[m] its detected weight and paths.  The same terms in another order: RTOL_SUM.
    Measured on the MI355X, largest relative difference of a cell over the 16 measurements: see DESIGN.md (sensitivity maps)"""
    make, dk = WALKS[which]
    p, spp, seed = make(), 16, 7
    base = dict(face=dk["face"], cos_min=0.3, t_min=T_MIN[which], t_bin=T_BIN)
    s, m, t = _array(ctx, p, dict(base, window=(0, 4, 0, 4)), (2, 2), GATES, False, spp, res=(8, 8, 8), seed=seed)
    assert s.shape == (1, GATES, 2, 2, 8, 8, 8, 3) and t[12] == 0 and t[0] == W * H * spp
    counts = m[..., 3]
    print(which, "detected per gate", counts.sum((1, 2)), "per detector", counts.sum(0).ravel())
    assert (counts.sum((1, 2)) > 16).sum() >= 2 and (counts.sum(0) > 16).sum() >= 3, "the gates of this walk hold too few paths: move T_MIN"
    worst = 0.0
    for g in range(GATES):
        for dv in range(2):
            for du in range(2):
                one, t1 = TS._render(ctx, p, dict(base, window=(2 * du, 2 * du + 2, 2 * dv, 2 * dv + 2), t_min=T_MIN[which] + g * T_BIN), spp, res=(8, 8, 8), seed=seed)
                np.testing.assert_allclose(s[0, g, dv, du], one, rtol=RTOL_SUM, atol=0)
                np.testing.assert_allclose(m[g, dv, du, :3], t1[1:4], rtol=RTOL_SUM, atol=0)
                assert m[g, dv, du, 3] == t1[8] and t1[12] == 0
                if one.any():
                    worst = max(worst, float((np.abs(s[0, g, dv, du] - one)[one != 0] / one[one != 0]).max()))
    print(which, "largest relative difference of a cell %.2e" % worst)


# ---- 2. one bin, one gate, scatter off ------------------------------------------------------------------------------------------------------

def test_one_bin_one_gate_is_the_single_detector_handle(ctx):
    make, dk = WALKS["straight homogeneous RGB"]
    p, gate = make(), dict(TS.CONE_GATE)
    one, t1 = TS._render(ctx, p, dict(dk, **gate), 16, res=(8, 8, 8), seed=7)
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.sensitivity_array_create((8, 8, 8), *CUBE, TS._det(sc, **dict(dk, **gate)))
    hm = ctx.sensitivity_array_create((8, 8, 8), *CUBE, TS._det(sc, **dict(dk, **gate)), (1, 1))
    hk = ctx.sensitivity_array_create((8, 8, 8), *CUBE, TS._det(sc, **dict(dk, **gate)), None, 1, True)
    try:
        ctx.render_sensitivity(sc, h, 0, 16, seed=7)
        s, m, t = ctx.sensitivity_read_array(h)
        assert s.shape == (1, 1, 1, 1, 8, 8, 8, 3) and ctx.sensitivity_shape(h) == (1, 1, 1, 0) and t1[8] > 64
        np.testing.assert_allclose(s[0, 0, 0, 0], one, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(t, t1, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(m[0, 0, 0, :3], t1[1:4], rtol=RTOL_SUM, atol=0)
        assert m[0, 0, 0, 3] == t1[8] and not m[0, 0, 0, 4:].any()
        s2, t2 = ctx.sensitivity_read(h)                                  # mer_sensitivity_read takes it
        assert np.array_equal(s2, s[0, 0, 0, 0]) and np.array_equal(t2, t)
        # ... and a handle of mer_sensitivity_create goes through mer_sensitivity_read_array and mer_sensitivity_shape
        h1 = ctx.sensitivity_create((8, 8, 8), *CUBE, TS._det(sc, **dict(dk, **gate)))
        try:
            ctx.render_sensitivity(sc, h1, 0, 16, seed=7)
            s3, m3, t3 = ctx.sensitivity_read_array(h1)
            assert ctx.sensitivity_shape(h1) == (1, 1, 1, 0)
        finally:
            ctx.sensitivity_destroy(h1)
        np.testing.assert_allclose(s3, s, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(m3, m, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(t3, t, rtol=RTOL_SUM, atol=0)
        # several measurements, or a scattering grid: mer_sensitivity_read refuses by name
        t16 = np.zeros(16)
        for bad in (hm, hk):
            with pytest.raises(capi.MerError, match="mer_sensitivity_read: .*use mer_sensitivity_read_array"):
                ctx.sensitivity_read(bad)
            assert ctx.lib.mer_sensitivity_read(ctx.h, C.c_int32(bad), None, t16.ctypes.data_as(C.c_void_p)) != 0
            assert "use mer_sensitivity_read_array" in ctx.lib.mer_last_error(ctx.h).decode()
    finally:
        for x in (h, hm, hk):
            ctx.sensitivity_destroy(x)
        for v in vols:
            v.destroy()


# ---- 3. the sums ----------------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["straight homogeneous RGB", "straight homogeneous RGB sphere", "trilinear Verlet", "acoustic RK4"])
def test_measurements_sum_to_the_totals(ctx, which):
    """a ragged box, scatter on: the measurements hold all of the detected weight and paths; the cells of K and the collisions outside the
    box hold all of w x collisions; the cells of J and the dropped length all of w x length"""
    make, dk = WALKS[which]
    s, m, t = _array(ctx, make(), dict(face=dk["face"], window=(0, 4, 0, 4), t_min=T_MIN[which], t_bin=1.0), (2, 2), 2, True, 16, res=RAGGED[0], box=RAGGED[1], seed=11)
    assert t[8] > 64 and t[12] == 0
    np.testing.assert_allclose(m[..., :3].reshape(-1, 3).sum(0), t[1:4], rtol=RTOL_SUM, atol=0)
    assert m[..., 3].sum() == t[8]
    lhs = s[1].reshape(-1, 3).sum(0) + t[13:16]
    print(which, "K cells + outside", lhs, "w x collisions", m[..., 4:7].reshape(-1, 3).sum(0), "outside", t[13:16])
    assert np.all(t[13:16] > 0) and np.all(t[4:7] > 0)
    np.testing.assert_allclose(lhs, m[..., 4:7].reshape(-1, 3).sum(0), rtol=RTOL_SUM, atol=0)
    np.testing.assert_allclose(s[0].reshape(-1, 3).sum(0) + t[4:7], t[9:12], rtol=RTOL_PIECE, atol=0)


# ---- 4. closed forms of K -------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["clear", "absorber"])
def test_nothing_scatters_k_is_zero(ctx, which):
    p = TE._clear(emitters=[_beam()]) if which == "clear" else TE._absorber(emitters=[_beam()])
    s, m, t = _array(ctx, p, dict(window=(0, 4, 0, 4)), (2, 2), 1, True, 16)
    assert t[8] > 64 and s[0].sum() > 0
    assert not s[1].any() and not m[..., 4:7].any() and not t[13:16].any()


SIGMA_S = 0.5
RAYS = {"straight homogeneous": "straight", "trilinear Verlet": "trilinear Verlet", "acoustic RK4": "acoustic RK4"}


@pytest.mark.parametrize("rays", list(RAYS))
def test_every_path_detected_k_is_sigma_t_times_the_collision_grid(ctx, rays):
    """The unit sphere, sigma_a = 0, sigma_s = 0.5 grey, strategy single with medium_sampling_weight 1, no roulette, no depth limit, the
    detector the sphere's whole raster: every path leaves with w = power, and at every collision the fluence grid deposits T power
    (transmittance / pdfSuccess) = power / sigma_t into the cell K takes w in: K = sigma_t x the raw sums of mer_render_fluence for the same
    scene, shard, seed and box, cell by cell up to the float32 arithmetic of the weights"""
    spp, seed = 4, 11
    p = TM.MEDIA["homogeneous"](emitters=[_beam()], strategy=P.STRATEGY_SINGLE, **TE._sphere(), **TM.RAYS[RAYS[rays]]())
    s, m, t = _array(ctx, p, dict(face=0, window=(0, 4, 0, 4)), None, 1, True, spp, res=RAGGED[0], box=RAGGED[1], seed=seed)
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    hf = ctx.fluence_create(RAGGED[0], *RAGGED[1])
    try:
        ctx.render_fluence(sc, hf, 0, spp, seed=seed)
        f, ft = ctx.fluence_read(hf)
    finally:
        ctx.fluence_destroy(hf)
        for v in vols:
            v.destroy()
    paths = W * H * spp
    assert t[0] == t[8] == ft[0] == paths and t[7] == 0 and ft[7] == 0 and t[12] == 0
    k = s[1, 0, 0, 0]
    assert np.array_equal(k != 0, f != 0) and (f != 0).any()
    rel = np.abs(k - SIGMA_S * f)[f != 0] / (SIGMA_S * f[f != 0])
    print(rays, "%d of %d values filled, largest relative difference of a cell %.2e; collisions per path %.2f, outside the box %.2f" %
          ((f != 0).sum(), f.size, rel.max(), m[0, 0, 0, 4] / POWER3[0] / paths, t[13] / POWER3[0] / paths))
    np.testing.assert_allclose(k, SIGMA_S * f, rtol=RTOL_PIECE, atol=0)
    np.testing.assert_allclose(t[13:16], SIGMA_S * ft[4:7], rtol=RTOL_PIECE, atol=0)
    assert np.all(t[13:16] > 0)


# ---- 5. against the float64 restatement -----------------------------------------------------------------------------------------------------

def test_scattering_cube_array_matches_float64(ctx):
    """16 batches of 16 384 paths against tests/sensitivity_array64.py (TA.array_ref): SCATTER's medium, 4^3 cells, face 5, the whole window in
    2 x 2 bins, two gates of width 1 from 4 on, K too.  Per cell under the project's bar for J and K of each gate-0 measurement and of gate 1
    summed over its detectors; every meas entry, every total and the 12 slab sums of every compared grid within 4 sigma.
    Measured on the MI355X (largest cell z, cells beyond 4 sigma, largest slab z, largest meas z, largest total z, fewest compared cells
    of 64): 3.23, 0, 3.37, 3.00, 2.18, 49; reference against reference on the CPU: 3.83, 0, 2.80, 2.52, 0.24, 49.
    The seeds are 1900 + j.  A first set, 900 + j, put one slab sum of 360 (K, gate 0, detector (1, 0), y < -0.5, red) at z 4.05 against the
    reference's seed 0 and at most 3.45 against three other seeds of the reference; 48 GPU batches pooled against 64 of the reference
    have 3.21 as their largest slab z (sensitivity maps, has the figures): with 16 batches z is t-distributed, and 4 is
    passed once in 900 entries"""
    spp, K = 64, TA.K_BATCHES
    assert W * H * spp == TA.REF_PATHS
    ref = TA.array_ref(0)
    p = TE._base(emitters=[_beam()], sigma_s=list(TA.SCATTER["sigma_s"]), sigma_a=list(TA.SCATTER["sigma_a"]), g=TA.SCATTER["g"])
    a = TA.REF_ARRAY
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.sensitivity_array_create((4, 4, 4), *CUBE, TS._det(sc, window=(0, 4, 0, 4), t_min=a["t_min"], t_bin=a["t_bin"]), a["bins"], a["gates"], True)
    got = []
    try:
        for j in range(K):
            ctx.sensitivity_clear(h)
            ctx.render_sensitivity(sc, h, 0, spp, seed=1900 + j)
            got.append(ctx.sensitivity_read_array(h))
    finally:
        ctx.sensitivity_destroy(h)
        for v in vols:
            v.destroy()
    s = np.array([g[0] for g in got])
    z = TA.check_array((s[:, 0], s[:, 1], np.array([g[1] for g in got]), np.array([g[2] for g in got])), ref, "GPU against float64")
    print("GPU against float64 (cell z, beyond 4 sigma, slab z, meas z, total z, fewest compared cells):", z)


# ---- 6. the derivative of the detected signal by sigma_s ------------------------------------------------------------------------------------

@pytest.mark.parametrize("which", ["straight", "curved"])
def test_k_and_j_give_the_derivative_by_sigma_s(ctx, which):
    """test_jacobian_is_minus_the_derivative_of_the_signal's set-up with sigma_s shifted by +- delta: strategy manual at a fixed density, no
    roulette, at most 20 flights, so the three renders walk the same paths, and per measurement (2 x 2 detectors of one raster cell, two
    gates of width 0.25; the signal from the time-resolved exitance map's frames and cells) the central difference of the signal equals
    sum(K) / sigma_s - sum(J) within DERIV_RTOL (sum(K) / sigma_s + sum(J)): tests/test_sensitivity_array64.py has the truncation bound.
    Curved (stepsize h): the last piece before the boundary deposits no length, at most 1.5 h per path, and K loses nothing, so the estimate
    may exceed the derivative by at most 1.5 h x the detected weight.  Measurements of more than 64 paths are checked"""
    D = DERIV
    h, spp, seed = 0.05, 64, 5
    t_min, t_bin = (4.5, 0.25) if which == "curved" else (4.0, 0.25)
    dk = dict(face=5, window=(1, 3, 1, 3), cos_min=0.2, t_min=t_min, t_bin=t_bin)
    curved = dict(rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=h, stepper=P.STEP_VERLET) if which == "curved" else {}

    def scene(shift):
        return TE._base(emitters=[_beam()], sigma_s=list(D["sigma_s"] + shift), sigma_a=list(D["sigma_a"]), g=D["g"], strategy=P.STRATEGY_MANUAL,
                        sampling_density=D["density"], medium_sampling_weight=D["weight"], rr_depth=D["rr_depth"], max_depth=D["max_depth"], **curved)

    def signal(shift):
        sc, vols = ctx.upload_scene(scene(shift), layout=capi.LAYOUT_DENSE)
        m, t = ctx.exitance(sc, (4, 4), spp, frames=2, t_min=t_min, t_bin=t_bin, cos_min=0.2, seed=seed)
        for v in vols:
            v.destroy()
        return m[:, 5, 1:3, 1:3], t                                     # [gate][dv][du][3]
    s, m, t = _array(ctx, scene(0.0), dk, (1, 1), 2, True, spp, seed=seed)
    wp, tp = signal(+D["delta"])
    wm, tm = signal(-D["delta"])
    w0, t0 = signal(0.0)
    assert tp[14] == tm[14] == t0[14] and tp[7] == tm[7] == t[7] == t0[7]      # the same paths left
    np.testing.assert_allclose(m[..., :3], w0, rtol=RTOL_SUM, atol=0)
    assert t[12] == 0 and not t[4:7].any() and not t[13:16].any()
    deriv = (wp - wm) / (2 * D["delta"])
    ks, js = s[1].sum((3, 4, 5)) / D["sigma_s"], s[0].sum((3, 4, 5))
    est, tol = ks - js, DERIV_RTOL * (ks + js)
    big = m[..., 3] > 64
    print(which, "paths per measurement", m[..., 3].ravel(), "checked", int(big.sum()))
    print(which, "(estimate - derivative) / tolerance", ((est - deriv) / tol)[big], "1.5 h w / tolerance", (1.5 * h * m[..., :3] / tol)[big])
    assert big.sum() >= 3
    if which == "straight":
        assert np.all(np.abs(est - deriv)[big] <= tol[big])
    else:
        assert np.all((est - deriv)[big] >= -tol[big]) and np.all((est - deriv)[big] <= (1.5 * h * m[..., :3] + tol)[big])


# ---- 7. launch shapes -----------------------------------------------------------------------------------------------------------------------

def test_a_render_of_two_chunks_equals_its_half_shards(ctx):
    """the curved clear scene of 32 x 32 x 65 paths of test_gpu_sensitivity.py, one more chunk than PT_PATHS_PER_LAUNCH_CURVED holds, into an
    array handle with the scattering grid"""
    p = TE._clear(rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=0.05, stepper=P.STEP_VERLET, emitters=[_beam()], w=32, h=32)
    kw = dict(det_kw=dict(window=(0, 4, 0, 4), t_min=4.0, t_bin=0.5), bins=(2, 2), gates=2, scatter=True, seed=2)
    whole = _array(ctx, p, spp=65, **kw)
    parts = [_array(ctx, p, spp=count, begin=begin, **kw) for begin, count in ((0, 32), (32, 33))]
    assert whole[2][0] == whole[2][8] == 32 * 32 * 65 > 65536 and whole[2][12] == 0 and whole[0][0].sum() > 0
    assert parts[0][2][0] == 32 * 32 * 32 and parts[1][2][0] == 32 * 32 * 33
    for q in range(3):
        np.testing.assert_allclose(parts[0][q] + parts[1][q], whole[q], rtol=RTOL_SUM, atol=0)


@pytest.mark.parametrize("w,h,spp", [(40, 24, 3), (1, 1, 1)])
def test_partial_tiles_and_a_single_path(ctx, w, h, spp):
    """a 40 x 24 film (two tiles, 960 of 2048 work ids per sample inside the image) and a render of one path: the clear cube's column
    in the measurement of the beam's raster cell (2, 2) -> detector (1, 1), gate 1 of [2.5, 3.5), [3.5, 4.5): the path length is 4"""
    s, m, t = _array(ctx, TE._clear(emitters=[_beam()], w=w, h=h), dict(window=(0, 4, 0, 4), t_min=2.5, t_bin=1.0), (2, 2), 2, True, spp)
    paths = w * h * spp
    assert t[0] == paths and t[8] == paths and t[12] == 0
    want = np.zeros((2, 2, 2)); want[1, 1, 1] = paths
    assert np.array_equal(m[..., 3], want)
    np.testing.assert_array_equal(m[1, 1, 1, :3], paths * POWER3)
    on = TS._column()
    assert not s[1].any() and not s[0, 0].any() and not s[0, 1, 0].any() and not s[0, 1, 1, 0].any() and np.all(s[0, 1, 1, 1][~on] == 0.0)
    np.testing.assert_allclose(s[0, 1, 1, 1][on], np.broadcast_to(paths * POWER3 * 0.5, (4, 3)), rtol=RTOL_PIECE, atol=0)


# ---- 8. the bounds-checking build -----------------------------------------------------------------------------------------------------------

def test_bounds_checking_build_agrees(ctx):
    cases = [WALKS[k] + (T_MIN[k],) for k in ("straight gridded sigma_t", "trilinear Verlet", "straight homogeneous RGB sphere")]
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for make, dk, t_min in cases:
            got = [_array(cx, make(), dict(face=dk["face"], window=(0, 4, 0, 4), cos_min=0.3, t_min=t_min, t_bin=0.5), (2, 2), 4, True, 16, res=RAGGED[0],
                          box=RAGGED[1], seed=3) for cx in (c, ctx)]
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (n, kind, idx, lim)
            assert got[0][0][0].sum() > 0 and got[0][0][1].sum() > 0 and got[0][2][8] > 0 and got[0][2][12] == 0 and (got[0][1][..., 3] > 0).sum() >= 6
            for q in range(3):
                np.testing.assert_allclose(got[0][q], got[1][q], rtol=RTOL_SUM, atol=0)
    finally:
        c.close()


# ---- 9. the library's refusals --------------------------------------------------------------------------------------------------------------

def test_library_refusals(ctx):
    """mer_sensitivity_array_create's checks past the Python front end: its own prefix, *out = 0, and the Python check gives the same message"""
    for kw, msg in ((dict(res=(0, 4, 4)), "res must lie in 1 ... 1024"), (dict(bmin=(1, -1, -1)), "bmin must be below bmax"),
                    (dict(boundary=P.BOUNDARY_SDF), "boundary must be the cube"), (dict(dres=(4, 5000)), "detector res must lie in 1 ... 4096"),
                    (dict(t_bin=-1.0), "t_bin must be finite and at least 0"), (dict(t_min=float("nan")), "t_min must be finite"),
                    (dict(cos_min=1.0), "cos_min must lie in"), (dict(det_reserved=1), "reserved must be 0"), (dict(face=6), "face must be one of"),
                    (dict(window=(0, 5, 0, 4)), "the window must lie inside the raster"), (dict(window=(2, 2, 0, 4)), "the window is empty"),
                    (dict(bins=(0, 2)), "bin_u and bin_v must be at least 1"), (dict(bins=(2, -2)), "bin_u and bin_v must be at least 1"),
                    (dict(bins=(3, 2)), "bin_u and bin_v must divide the window"), (dict(bins=(2, 3)), "bin_u and bin_v must divide the window"),
                    (dict(gates=0), "gates must be at least 1"), (dict(gates=2), "several gates need t_bin > 0"),
                    (dict(scatter=2), "scatter must be 0 or 1"), (dict(reserved=(0, 7)), "reserved must be 0"),
                    (dict(res=(512, 512, 256), bins=(2, 2), scatter=1), r"more than 2\^27 cells x measurements x \(1 \+ scatter\)")):
        kw = dict(kw)
        det = capi.detector_desc(kw.pop("boundary", P.BOUNDARY_AABB), kw.pop("dres", (4, 4)), kw.pop("face", 5), kw.pop("window", (0, 4, 0, 4)),
                                 kw.pop("cos_min", 0.0), kw.pop("t_min", 0.0), kw.pop("t_bin", 0.0))
        det.reserved = kw.pop("det_reserved", 0)
        d = capi.sensitivity_array_desc(kw.pop("res", (4, 4, 4)), kw.pop("bmin", (-1, -1, -1)), kw.pop("bmax", (1, 1, 1)), det, kw.pop("bins", (2, 2)),
                                        kw.pop("gates", 1))
        d.scatter = kw.pop("scatter", 0)
        d.reserved[:] = kw.pop("reserved", (0, 0))
        assert not kw
        out = C.c_int32(-1)
        assert ctx.lib.mer_sensitivity_array_create(ctx.h, C.byref(d), C.byref(out)) != 0 and out.value == 0
        err = ctx.lib.mer_last_error(ctx.h).decode()
        assert err.startswith("mer_sensitivity_array_create: ") and re.search(msg, err), err
        with pytest.raises(capi.MerError, match=msg):
            capi.validate_sensitivity_array(d)
    shape = (C.c_int32 * 4)()
    assert ctx.lib.mer_sensitivity_shape(ctx.h, C.c_int32(12345), shape) != 0
    assert "mer_sensitivity_shape: unknown sensitivity handle" in ctx.lib.mer_last_error(ctx.h).decode()
    t16 = np.zeros(16)
    assert ctx.lib.mer_sensitivity_read_array(ctx.h, C.c_int32(12345), None, None, t16.ctypes.data_as(C.c_void_p)) != 0
    assert "mer_sensitivity_read_array: unknown sensitivity handle" in ctx.lib.mer_last_error(ctx.h).decode()


# ---- 10. the command line -------------------------------------------------------------------------------------------------------------------

def test_mer_render_writes_the_python_calls_grids(ctx, tmp_path):
    """mer_render --sensitivity=8,8,8 --detector=F,4,4,0,4,0,4 --detector-bins=2,2 --gate=0,32 --gates=2 --scatter on
    scenes/cfg_laser_clear.xml: the .npy of (J, K) / paths that Context.sensitivity_array gives, and its lines per measurement"""
    scene = os.path.join(ROOT, "scenes", "cfg_laser_clear.xml")
    defines = {"samples": "1", "sigmaS": "0.8", "sigmaA": "0.05"}
    out = str(tmp_path / "jk.npy")
    d, spp = host.flatten_xml(scene, defines)
    m0, te = ctx.exitance(d, (4, 4), spp, seed=3)
    face = int(np.argmax(m0[0].sum((1, 2, 3))))                             # the face most of the light leaves through
    args = [os.path.join(ROOT, "mitsubaer_amd", "mer_render"), "--sensitivity=8,8,8", "--detector=%d,4,4,0,4,0,4" % face, "--detector-bins=2,2", "--gate=0,32",
            "--gates=2", "--scatter", "--seed", "3", "-o", out]
    for k, v in defines.items():
        args += ["-D", "%s=%s" % (k, v)]
    r = subprocess.run(args + [scene], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "paths %d " % (128 * 96) in r.stdout and "disagreements 0" in r.stdout
    data = np.load(out)
    assert data.shape == (2, 2, 2, 2, 8, 8, 8, 3) and data.dtype == np.float32
    j, k, meas, info = ctx.sensitivity_array(d, (8, 8, 8), dict(res=(4, 4), face=face, t_min=0.0, t_bin=32.0), (2, 2), 2, spp, scatter=True, seed=3)
    assert info["paths"] == 128 * 96 and info["detected"] > 0 and j.sum() > 0 and k.sum() > 0
    np.testing.assert_allclose(data[0], j.astype(np.float32), rtol=1e-6, atol=0)
    np.testing.assert_allclose(data[1], k.astype(np.float32), rtol=1e-6, atol=0)
    lines = re.findall(r"measurement gate (\d+) dv (\d+) du (\d+)  detected (\d+)  weight (\S+) (\S+) (\S+)", r.stdout)
    assert len(lines) == 8
    for g, dv, du, n, a, b, c in lines:
        assert int(n) == meas[int(g), int(dv), int(du), 3]
        np.testing.assert_allclose([float(a), float(b), float(c)], meas[int(g), int(dv), int(du), :3], rtol=1e-6)
