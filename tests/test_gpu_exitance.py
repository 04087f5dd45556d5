"""The exitance map recorded from light paths (mer_render_exitance, mer_exitance.hpp) on the GPU: against closed forms (Beer-Lambert on the
beam's cell, exact zeros elsewhere, the solid angles of the cube's face cells, the equal-area cells of the sphere), the identity
sum(sums) + missed + rejected + late = escaped, the collision grid's walk (counters and totals), the float64 restatement
tests/exitance64.py per cell, causality of the timed map, a float64 eikonal trace on curved rays, and the interface: shards, clear /
accumulate, the bounds-checking build, the refusals, `mer_render --exitance`.

Set-up (tests/test_exitance64.py): a 16 x 16 film (path enumeration only) x 64 samples = 16 384 paths per batch, K = 16 batches with seeds
s0 + j, the cube [-1, 1]^3 or the unit sphere, the beam of power 5 from (0.2, 0.1, -3) along +z, maps of 4 x 4 cells per face.
medium_sampling_weight = 1 throughout.  Statistics: the project's bar -- at most 1 + 1 % of the cells beyond 4 sigma, totals within 4 sigma."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host
from tests import scenes
from tests import exitance64 as E
from tests import test_exitance64 as T
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
ST = T.SIGMA_S + T.SIGMA_A
RTOL_SUM = 1e-9          # one set of deposits added in two orders: at most 2^20 float64 adds per cell, each within 2^-53: 2^-33 = 1.2e-10, rounded up
INTENSITY = 2.0          # of the point emitters: 4 pi I per path


def _beam(o=BEAM_O, d=BEAM_D, power=T.POWER):
    return P.collimated_emitter(TP._beam_frame(o, d), [power] * 3)


def _base(**kw):
    base = dict(w=W, h=H, fov_x_deg=40.0, cam_to_world=CAM, phase=P.PHASE_HG, g=T.G, sigma_s=[T.SIGMA_S] * 3, sigma_a=[T.SIGMA_A] * 3,
                env_radiance=[0, 0, 0], rfilter=P.FILTER_BOX, rfilter_param=0.5, integrator=P.INTEGRATOR_PTRACER, medium_sampling_weight=1.0,
                rr_depth=5, emitters=[_beam()])
    base.update(kw)
    return scenes.homogeneous_scene(**base)


def _absorber(**kw):
    return _base(sigma_s=[0.0] * 3, sigma_a=[T.ABSORBER] * 3, g=0.0, **kw)


def _grid(**kw):
    """a gridded sigma_t over the cube"""
    base = dict(sigma_mode=P.SIGMA_GRID, density=np.ones((16, 16, 16), np.float32), density_scale=ST, albedo=[T.SIGMA_S / ST] * 3)
    base.update(kw)
    return _base(**base)


def _clear(**kw):
    """no extinction anywhere: a 2^3 density grid of zeros"""
    return _grid(density=np.zeros((2, 2, 2), np.float32), density_scale=1.0, albedo=[0.0] * 3, **kw)


def _sphere(**kw):
    return dict(boundary=P.BOUNDARY_SPHERE, sph_center=[0.0, 0.0, 0.0], sph_radius=T.RADIUS, **kw)


def _batches(ctx, p, seed0, res=T.RES, k=K, **desc):
    """k batches with seeds seed0 + j into one map, cleared in between: raw sums (k, frames, faces, res_v, res_u, 3), totals (k, 16)"""
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.exitance_create(sc.boundary, res, **desc)
    sums, totals = [], []
    try:
        for j in range(k):
            ctx.exitance_clear(h)
            ctx.render_exitance(sc, h, 0, SPP, seed=seed0 + j)
            s, t = ctx.exitance_read(h)
            assert np.isfinite(s).all() and np.isfinite(t).all() and t[15] == 0
            sums.append(s); totals.append(t)
    finally:
        ctx.exitance_destroy(h)
        for v in vols:
            v.destroy()
    return np.array(sums), np.array(totals)


def _grey(sums):
    """a grey scene: the three channels hold the same sums (their atomics add in their own order); returns channel 0"""
    np.testing.assert_allclose(sums[..., 1], sums[..., 0], rtol=RTOL_SUM, atol=0)
    np.testing.assert_allclose(sums[..., 2], sums[..., 0], rtol=RTOL_SUM, atol=0)
    return sums[..., 0]


def _identity(sums, tot, rtol=1e-12):
    """sum(sums) + missed + rejected + late == escaped, per batch and channel"""
    for c in range(3):
        lhs = sums[..., c].reshape(len(sums), -1).sum(1) + tot[:, 4 + c] + tot[:, 11 + c] + tot[:, 8 + c]
        np.testing.assert_allclose(lhs, tot[:, 1 + c], rtol=rtol, atol=0)


# ---- 1. pure absorber, the beam's cell -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1.0, 1.4])
def test_pure_absorber_beam_lands_in_one_cell(ctx, n):
    """the cell of face +z under the beam holds P e^{-2 sigma_a} per path under the binomial variance, every other cell of every face is
    exactly 0; timed: the same deposit in the single frame that holds the exterior leg 2 + 2 rif_const, exactly 0 elsewhere"""
    p = _absorber(rif_const=n)
    sums, tot = _batches(ctx, p, 100)
    g = _grey(sums)
    assert g.shape == (K, 1, 6, 4, 4)
    on = np.zeros((1, 6, 4, 4), bool); on[0, T.BEAM_FACE, T.BEAM_IV, T.BEAM_IU] = True
    assert np.all(g[:, ~on] == 0.0), "exits off the beam's cell"
    pe = np.exp(-2 * T.ABSORBER)
    cellsum = g[:, 0, T.BEAM_FACE, T.BEAM_IV, T.BEAM_IU]
    z = abs(cellsum.mean() - PATHS * T.POWER * pe) / np.sqrt(PATHS * T.POWER ** 2 * pe * (1 - pe) / K)          # the binomial variance
    print("beam cell, n %.1f: mean / ref %.5f, z %.2f" % (n, cellsum.mean() / (PATHS * T.POWER * pe), z))
    assert z <= 4
    np.testing.assert_array_equal(cellsum, tot[:, 1])                     # sums of P, exact in float64: all that escapes is in the cell
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:14] == 0)
    np.testing.assert_array_equal(tot[:, 14] * T.POWER, cellsum)
    # timed, the seeds of the steady map: the same paths
    frames, t_min, t_bin = 8, 2.15, 0.5
    f = int(np.floor((2.0 + 2.0 * n - t_min) / t_bin))
    assert 0 < f < frames - 1 and abs((2.0 + 2.0 * n - t_min) / t_bin - f - 0.5) < 0.25         # well inside its frame
    ts, tt = _batches(ctx, p, 100, k=4, frames=frames, t_min=t_min, t_bin=t_bin)
    gt = _grey(ts)
    onf = np.zeros((frames, 6, 4, 4), bool); onf[f, T.BEAM_FACE, T.BEAM_IV, T.BEAM_IU] = True
    assert np.all(gt[:, ~onf] == 0.0) and np.all(tt[:, 8:11] == 0)
    np.testing.assert_array_equal(gt[:, f, T.BEAM_FACE, T.BEAM_IV, T.BEAM_IU], cellsum[:4])


# ---- 2. clear cube, point emitter at the centre ----------------------------------------------------------------------------------------

def test_clear_cube_cells_hold_their_solid_angle(ctx):
    p = _clear(emitters=[P.point_emitter([0, 0, 0], [INTENSITY] * 3)])
    sums, tot = _batches(ctx, p, 200)
    g = _grey(sums)[:, 0]
    om = np.broadcast_to(E.cube_cell_solid_angles(T.RES), (6, 4, 4))
    phi = 4 * np.pi * INTENSITY
    pc = om / (4 * np.pi)
    E.bar(g.mean(0), np.sqrt(PATHS * phi ** 2 * pc * (1 - pc) / K), PATHS * INTENSITY * om, what="clear cube cells")
    # nothing is lost: the six faces hold all that was emitted
    _identity(sums, tot)
    assert np.all(tot[:, 4:14] == 0) and np.all(tot[:, 14] == PATHS)
    np.testing.assert_allclose(g.reshape(K, -1).sum(1), tot[:, 1], rtol=1e-12, atol=0)
    np.testing.assert_allclose(tot[:, 1], PATHS * phi, rtol=1e-6, atol=0)           # the power of a path is a float32
    # the cone cos >= 0.8 about a face normal lies inside the face: 2 pi (1 - 0.8) I per face
    cs, ct = _batches(ctx, p, 200, cos_min=0.8)
    acc = 6 * 2 * np.pi * 0.2 * INTENSITY
    pa = acc / phi
    accepted = _grey(cs).reshape(K, -1).sum(1)
    E.total_bar(accepted, PATHS * acc, what="accepted")
    E.total_bar(ct[:, 11], PATHS * (phi - acc), what="rejected")
    assert abs(accepted.mean() / (PATHS * acc) - 1) < 4 * np.sqrt((1 - pa) / (pa * PATHS * K))
    _identity(cs, ct)
    np.testing.assert_array_equal(ct[:, 1], tot[:, 1])                    # the same paths
    assert np.all(_grey(cs)[:, 0] <= g * (1 + RTOL_SUM))                   # the cone only removes exits


# ---- 3. pure absorber sphere, point emitter at the centre ------------------------------------------------------------------------------

def test_absorber_sphere_cells_are_equal_area(ctx):
    p = _absorber(emitters=[P.point_emitter([0, 0, 0], [INTENSITY] * 3)], **_sphere())
    sums, tot = _batches(ctx, p, 300)
    g = _grey(sums)
    assert g.shape == (K, 1, 1, 4, 4)
    phi = 4 * np.pi * INTENSITY
    pc = np.exp(-T.ABSORBER * T.RADIUS) / 16
    E.bar(g[:, 0, 0].mean(0), np.full((4, 4), np.sqrt(PATHS * phi ** 2 * pc * (1 - pc) / K)), np.full((4, 4), PATHS * phi * pc), what="sphere cells")
    _identity(sums, tot)


# ---- 4. the identity -------------------------------------------------------------------------------------------------------------------

def test_every_escaping_path_lands_in_exactly_one_total(ctx):
    """a scattering cube lit by a point emitter outside it (part of its rays miss), cos_min = 0.5, a window that cuts the tail"""
    em = [P.point_emitter(T.OUTSIDE_POINT["o"], [INTENSITY] * 3)]
    desc = dict(frames=8, t_min=0.5, t_bin=0.5, cos_min=0.5)
    sums, tot = _batches(ctx, _base(emitters=em, rif_const=1.33), 400, k=4, **desc)
    assert np.all(tot[:, 4] > 0) and np.all(tot[:, 8] > 0) and np.all(tot[:, 11] > 0) and np.all(tot[:, 14] > 0) and np.all(tot[:, 7] == 0)
    _identity(sums, tot)
    # weight-1 settings: albedo 1 and the roulette out of reach: every exit weighs the power w of a path, so the totals are counts
    sums, tot = _batches(ctx, _base(emitters=em, sigma_a=[0.0] * 3, rr_depth=10 ** 6), 450, k=4, **desc)
    _identity(sums, tot)
    assert np.all(tot[:, 7] == 0)
    w = float(np.float32(4 * np.pi * INTENSITY))
    g = _grey(sums)
    for j in range(4):
        wj = g[j].sum() / tot[j, 14]
        assert abs(wj / w - 1) < 1e-6
        counts = tot[j, [4, 11, 8]] / wj                                   # missed, rejected, late
        np.testing.assert_allclose(counts, np.round(counts), rtol=1e-5, atol=0)       # a weight is P after up to ~100 float32 roundings of T, 6e-8 each
        assert tot[j, 14] == PATHS - np.round(counts).sum()               # every path that met the cube left it again


# ---- 5. the collision grid's walk ------------------------------------------------------------------------------------------------------

def _rif():
    yy = np.linspace(-1, 1, 16)
    return np.broadcast_to((TP.RIF_A + TP.RIF_B * yy)[None, :, None], (16, 16, 16)).astype(np.float32).copy()


@pytest.mark.parametrize("which", ["straight homogeneous", "curved gridded"])
def test_same_walk_as_the_collision_grid(ctx, which):
    """counters entry for entry; paths, escaped and ended bit-equal.  The escaped sums do not depend on the order of their atomics: a weight is
    a float32 in [3, 5.3] (P albedo^k below rr_depth 5, P T / q >= 0.68 P after it), a multiple of 2^-22, and 16 384 of them stay below
    2^17: 39 bits, exact in float64"""
    p = _base() if which == "straight homogeneous" else _grid(rif_mode=P.RIF_TRILINEAR, rif=_rif(), stepsize=0.05, stepper=P.STEP_VERLET)
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    got = []
    hf = ctx.fluence_create((8, 8, 8), (-1, -1, -1), (1, 1, 1))
    he = ctx.exitance_create(sc.boundary, T.RES, frames=4, t_min=2.0, t_bin=1.0, cos_min=0.3)
    try:
        ctx.counters_reset()
        ctx.render_fluence(sc, hf, 0, SPP, seed=7)
        got.append((ctx.counters(), ctx.fluence_read(hf)[1]))
        ctx.counters_reset()
        ctx.render_exitance(sc, he, 0, SPP, seed=7)
        got.append((ctx.counters(), ctx.exitance_read(he)[1]))
    finally:
        ctx.fluence_destroy(hf); ctx.exitance_destroy(he)
        for v in vols:
            v.destroy()
    (ca, ta), (cb, tb) = got
    print("collision", list(ca), ta, "exitance", list(cb), tb)
    assert ca[capi.C_PATHS] == PATHS and ca[capi.C_REAL] > PATHS
    assert list(ca) == list(cb)
    assert ta[0] == tb[0] == PATHS and ta[7] == tb[7]
    np.testing.assert_array_equal(tb[1:4], ta[1:4])
    assert tb[8] > 0 and tb[11] > 0 and tb[14] > 0                          # the window and the cone were at work


# ---- 6. against the float64 restatement ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape", ["cube", "sphere"])
def test_scattering_medium_matches_float64(ctx, shape):
    r, rt, hits = T.scattering_ref(shape)
    assert hits.min() >= 16, "the reference must fill every cell of every face"
    sums, tot = _batches(ctx, _base(**(_sphere() if shape == "sphere" else {})), 500 if shape == "cube" else 550)
    g = _grey(sums)
    assert g.shape == r.shape
    E.bar(g.mean(0), g.std(0, ddof=1) / np.sqrt(K), r.mean(0), r.var(0, ddof=1) / K, what=shape + " cells")
    for f in range(g.shape[2]):
        a, b = g[:, 0, f].sum((1, 2)), r[:, 0, f].sum((1, 2))
        E.total_bar(a, b.mean(), b.var(ddof=1) / K, what="%s face %d" % (shape, f))
    E.total_bar(tot[:, 1], rt[:, 1].mean(), rt[:, 1].var(ddof=1) / K, what=shape + " escaped")
    E.total_bar(tot[:, 14], rt[:, 14].mean(), rt[:, 14].var(ddof=1) / K, what=shape + " exits")
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 7] == 0) and np.all(tot[:, 4:14] == 0)
    _identity(sums, tot)


# ---- 7. causality ----------------------------------------------------------------------------------------------------------------------

def test_no_light_arrives_before_the_straight_line(ctx):
    n, frames, t_min, t_bin = 1.33, 24, 2.0, 0.25
    p = _base(rif_const=n)
    ts, tt = _batches(ctx, p, 600, k=2, frames=frames, t_min=t_min, t_bin=t_bin)
    ss, st = _batches(ctx, p, 600, k=2)
    gt, gs = _grey(ts), _grey(ss)
    entry = np.array([BEAM_O[0], BEAM_O[1], -1.0])
    ends = t_min + (np.arange(frames) + 1) * t_bin
    checked = 0
    for face in range(6):
        for iv in range(4):
            for iu in range(4):
                lo, hi = E.cell_rect(face, iv, iu, T.RES)
                lmin = 2.0 + n * np.linalg.norm(entry - np.clip(entry, lo, hi))
                early = ends < lmin - t_bin
                checked += early.sum()
                assert np.all(gt[:, early, face, iv, iu] == 0.0), (face, iv, iu)
    assert checked > 6 * 16 * 2
    beam = gt[:, :, T.BEAM_FACE, T.BEAM_IV, T.BEAM_IU].sum(0)
    assert np.flatnonzero(beam)[0] == int(np.floor((2.0 + 2.0 * n - t_min) / t_bin))
    # the window cuts the tail: what it holds plus `late` is the steady map of the same seeds
    assert np.all(tt[:, 8] > 0)
    np.testing.assert_allclose(gt.reshape(2, -1).sum(1) + tt[:, 8], gs.reshape(2, -1).sum(1), rtol=RTOL_SUM, atol=0)
    assert np.all(gt.sum(1) <= gs[:, 0] * (1 + RTOL_SUM))
    np.testing.assert_array_equal(tt[:, [0, 7]], st[:, [0, 7]])
    np.testing.assert_allclose(tt[:, 1:4], st[:, 1:4], rtol=RTOL_SUM, atol=0)


# ---- 8. curved rays, clear medium ------------------------------------------------------------------------------------------------------

CURVED_O = [0.25, -0.5, -3.0]


def _curved_trace(h=0.002):
    """the beam from CURVED_O through n = RIF_A + RIF_B y in float64 (RK4): the exit point on the cube and the optical length
    exterior leg + integral n ds (trapezoid over the steps; the last step is shortened by bisection)"""
    def nn(q):
        return TP.RIF_A + TP.RIF_B * q[1]
    p = np.array([CURVED_O[0], CURVED_O[1], -1.0]); v = np.array(BEAM_D) * nn(p)
    opt = 2.0
    for _ in range(100000):
        q, w = TP._rk4(p, v, h)
        if np.all(np.abs(q) <= 1):
            opt += 0.5 * h * (nn(p) + nn(q)); p, v = q, w
            continue
        lo, hi = 0.0, h
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if np.all(np.abs(TP._rk4(p, v, mid)[0]) <= 1):
                lo = mid
            else:
                hi = mid
        q, _w = TP._rk4(p, v, lo)
        return q, opt + 0.5 * lo * (nn(p) + nn(q))
    raise AssertionError("the beam never left the cube")


@pytest.mark.parametrize("stepper", [P.STEP_VERLET, P.STEP_RK4])
def test_curved_clear_beam_exits_where_the_float64_trace_does(ctx, stepper):
    """n = 1.3 + 0.15 y on a 16^3 dense grid, zero density, stepsize 0.05: all of the weight, P per path, lands in the face, cell and frame
    the float64 trace predicts"""
    h, n_max = 0.05, TP.RIF_A + TP.RIF_B
    frames, t_min, t_bin = 5, 3.0, 0.6
    x, length = _curved_trace()
    face = int(E.cell(x[None], E.CUBE, T.RES)[0]) // 16
    iv, iu = divmod(int(E.cell(x[None], E.CUBE, T.RES)[0]) % 16, 4)
    assert face == 5
    fu, fv = (x[0] + 1) / 2 * 4, (x[1] + 1) / 2 * 4
    assert min(fu - iu, iu + 1 - fu, fv - iv, iv + 1 - fv) >= 0.25            # a quarter cell from the cell's edges
    fl = (length - t_min) / t_bin
    fr = int(np.floor(fl))
    assert 0 <= fr < frames and min(fl - fr, fr + 1 - fl) * t_bin >= 2 * h * n_max and t_bin >= 8 * h * n_max
    assert abs(x[1] - CURVED_O[1]) > 0.2                                      # the beam bends by more than a third of a cell
    p = _clear(rif_mode=P.RIF_TRILINEAR, rif=_rif(), stepsize=h, stepper=stepper, emitters=[_beam(CURVED_O)])
    sums, tot = _batches(ctx, p, 700 + stepper, k=2, frames=frames, t_min=t_min, t_bin=t_bin)
    g = _grey(sums)
    on = np.zeros((frames, 6, 4, 4), bool); on[fr, face, iv, iu] = True
    print("stepper %d: exit %s, optical length %.5f -> frame %d, face %d, cell (%d, %d)" % (stepper, x, length, fr, face, iv, iu))
    assert np.all(g[:, ~on] == 0.0)
    np.testing.assert_array_equal(g[:, fr, face, iv, iu], PATHS * T.POWER)
    assert np.all(tot[:, 1:4] == PATHS * T.POWER) and np.all(tot[:, 4:14] == 0) and np.all(tot[:, 14] == PATHS)


# ---- 9., 10. curved = straight, gridded = homogeneous ----------------------------------------------------------------------------------

_CACHE = {}


def _straight_133(ctx):
    if "s" not in _CACHE:
        _CACHE["s"] = _batches(ctx, _base(rif_const=1.33), 800, frames=6, t_min=2.0, t_bin=1.5, cos_min=0.2)
    return _CACHE["s"]


def _compare(a, ta, b, tb, what, frames=True):
    ga, gb = _grey(a).sum(1), _grey(b).sum(1)                                 # per cell over the window: every cell is filled (test 6)
    E.bar(ga.mean(0), ga.std(0, ddof=1) / np.sqrt(K), gb.mean(0), gb.var(0, ddof=1) / K, what=what + " cells")
    if frames:
        fa, fb = _grey(a).sum((2, 3, 4)), _grey(b).sum((2, 3, 4))             # per frame over the boundary
        E.bar(fa.mean(0), fa.std(0, ddof=1) / np.sqrt(K), fb.mean(0), fb.var(0, ddof=1) / K, what=what + " frames")
    for q, name in ((1, "escaped"), (8, "late"), (11, "rejected"), (14, "exits")):
        E.total_bar(ta[:, q], tb[:, q].mean(), tb[:, q].var(ddof=1) / K, what="%s %s" % (what, name))
    assert np.all(ta[:, 7] == 0)
    _identity(a, ta)


@pytest.mark.parametrize("stepper", [P.STEP_VERLET, P.STEP_RK4])
def test_constant_rif_grid_matches_rif_const(ctx, stepper):
    """a constant 1.33 index grid through the curved kernels against rif_const = 1.33 through the straight ones, with a cone, per cell over
    the window.  Not per frame: a curved exit's path length lacks the piece between the last point inside and the boundary (mer.h), h n / 2 =
    0.033 on average at h = 0.05, which moves 1.5 % of the exits near a frame's edge into the earlier frame -- measured per frame over the
    boundary, curved / straight: 8732 / 8457, 27791 / 27214, 13652 / 14393 (z 4.6, 7.7, 9.9 with these 262 144 paths), the same for both
    steppers.  The frame a curved path lands in is pinned by test_curved_clear_beam_exits_where_the_float64_trace_does"""
    rif = np.full((16, 16, 16), 1.33, np.float32)
    a, ta = _batches(ctx, _base(rif_mode=P.RIF_TRILINEAR, rif=rif, stepsize=0.05, stepper=stepper), 900 + stepper, frames=6, t_min=2.0, t_bin=1.5, cos_min=0.2)
    b, tb = _straight_133(ctx)
    _compare(a, ta, b, tb, "curved %d vs straight" % stepper, frames=False)


def test_gridded_sigma_matches_homogeneous(ctx):
    a, ta = _batches(ctx, _grid(rif_const=1.33), 1000, frames=6, t_min=2.0, t_bin=1.5, cos_min=0.2)
    b, tb = _straight_133(ctx)
    _compare(a, ta, b, tb, "grid vs homogeneous")


# ---- 11. shards, clear, accumulate -----------------------------------------------------------------------------------------------------

def test_half_shards_add_up_and_the_map_accumulates(ctx):
    sc, _ = ctx.upload_scene(_base())
    h = ctx.exitance_create(sc.boundary, T.RES, frames=4, t_min=2.0, t_bin=1.0, cos_min=0.3)
    try:
        ctx.render_exitance(sc, h, 0, SPP, seed=9)
        whole, tw = ctx.exitance_read(h)
        parts = []
        for begin in (0, 32):
            ctx.exitance_clear(h)
            z, tz = ctx.exitance_read(h)
            assert not z.any() and not tz.any()
            ctx.render_exitance(sc, h, begin, 32, seed=9)
            parts.append(ctx.exitance_read(h))
        assert parts[0][1][0] == parts[1][1][0] == PATHS // 2 and tw[0] == PATHS
        assert parts[0][0].sum() > 0 and not np.array_equal(parts[0][0], parts[1][0])
        np.testing.assert_allclose(parts[0][0] + parts[1][0], whole, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(parts[0][1] + parts[1][1], tw, rtol=RTOL_SUM, atol=0)
        assert parts[0][1][14] + parts[1][1][14] == tw[14] > 0
        ctx.render_exitance(sc, h, 0, 32, seed=9)
        both, tb = ctx.exitance_read(h)
        np.testing.assert_allclose(both, whole, rtol=RTOL_SUM, atol=0)
        assert tb[0] == PATHS and tb[14] == tw[14]
        _, t_only = ctx.exitance_read(h, sums=False)
        assert np.array_equal(t_only, tb)
        # the convenience call: one map, created and destroyed
        s2, t2 = ctx.exitance(sc, T.RES, SPP, frames=4, t_min=2.0, t_bin=1.0, cos_min=0.3, seed=9)
        np.testing.assert_allclose(s2, whole, rtol=RTOL_SUM, atol=0)
        assert t2[0] == PATHS
    finally:
        ctx.exitance_destroy(h)


# ---- 12. the bounds-checking build -----------------------------------------------------------------------------------------------------

def test_bounds_checking_build_agrees(ctx):
    cases = (_grid(rif_const=1.33), _base(rif_mode=P.RIF_TRILINEAR, rif=_rif(), stepsize=0.05, stepper=P.STEP_VERLET), _base(**_sphere()))
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for p in cases:
            got = []
            for cx in (c, ctx):
                sc, vols = cx.upload_scene(p, layout=capi.LAYOUT_DENSE)
                got.append(cx.exitance(sc, (5, 3), SPP, frames=7, t_min=2.0, t_bin=0.7, cos_min=0.1, seed=3))
                for v in vols:
                    v.destroy()
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (n, kind, idx, lim)
            assert got[0][0].sum() > 0 and got[0][1][14] > 0
            np.testing.assert_allclose(got[0][0], got[1][0], rtol=RTOL_SUM, atol=0)
            np.testing.assert_allclose(got[0][1], got[1][1], rtol=RTOL_SUM, atol=0)
            assert got[0][1][0] == got[1][1][0] == PATHS
    finally:
        c.close()


# ---- 13. refusals ----------------------------------------------------------------------------------------------------------------------

def test_library_refusals(ctx):
    """mer_render_exitance's own checks (the Python front end's are bypassed by editing the flat scene); nothing is launched"""
    h = ctx.exitance_create(P.BOUNDARY_AABB, T.RES)
    hf = ctx.fluence_create((4, 4, 4), (-1, -1, -1), (1, 1, 1))

    def desc(**kw):
        return ctx.upload_scene(_base(**kw))[0]

    def refused(sc, msg, handle=None):
        with pytest.raises(capi.MerError, match=msg):
            ctx.render_exitance(sc, h if handle is None else handle, 0, 1)
    try:
        sc = desc(); sc.integrator = P.INTEGRATOR_VOLPATH
        refused(sc, "mer_render_exitance: the scene's integrator must be ptracer")
        refused(desc(**_sphere()), "the scene's boundary differs from the map's")
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
        # handles: the two kinds do not mix
        refused(desc(), "mer_render_exitance: unknown exitance handle", handle=hf)
        refused(desc(), "unknown exitance handle", handle=h + 1000)
        with pytest.raises(capi.MerError, match="mer_render_fluence: unknown fluence handle"):
            ctx.render_fluence(desc(), h, 0, 1)
        for call, handle, msg in ((ctx.exitance_clear, hf, "unknown exitance handle"), (ctx.exitance_destroy, hf, "unknown exitance handle"),
                                  (ctx.fluence_clear, h, "unknown fluence handle"), (ctx.fluence_destroy, h, "unknown fluence handle"),
                                  (ctx.exitance_clear, h + 1000, "unknown exitance handle"), (ctx.exitance_destroy, h + 1000, "unknown exitance handle")):
            with pytest.raises(capi.MerError, match=msg):
                call(handle)
        t16 = np.zeros(16)
        for bad in (hf, 0, h + 1000):
            assert ctx.lib.mer_exitance_read(ctx.h, C.c_int32(bad), None, t16.ctypes.data_as(C.c_void_p)) != 0
            assert "unknown exitance handle" in ctx.lib.mer_last_error(ctx.h).decode()
        assert ctx.lib.mer_fluence_read(ctx.h, C.c_int32(h), None, t16.ctypes.data_as(C.c_void_p)) != 0
        assert "unknown fluence handle" in ctx.lib.mer_last_error(ctx.h).decode()
        # nothing was launched: both are still zero
        s, t = ctx.exitance_read(h)
        assert not s.any() and not t.any()
        s, t = ctx.fluence_read(hf)
        assert not s.any() and not t.any()
        # descs, past the Python check
        for kw, msg in ((dict(boundary=P.BOUNDARY_SDF), "boundary must be the cube"), (dict(res=(0, 4)), "res must lie in 1 ... 4096"),
                        (dict(res=(4, 5000)), "res must lie in 1 ... 4096"), (dict(frames=0, t_bin=0.5), "frames must lie in 1 ... 4096"),
                        (dict(frames=4097, t_bin=0.5), "frames must lie in 1 ... 4096"), (dict(t_bin=-1.0), "t_bin must be finite and at least 0"),
                        (dict(t_bin=float("inf")), "t_bin must be finite and at least 0"), (dict(frames=2), "a steady map \\(t_bin == 0\\) has one frame"),
                        (dict(t_min=float("nan")), "t_min must be finite"), (dict(cos_min=1.0), "cos_min must lie in"), (dict(cos_min=-0.5), "cos_min must lie in"),
                        (dict(reserved=1), "reserved must be 0"), (dict(res=(4096, 4096), frames=2, t_bin=0.5), "2\\^27")):
            kw = dict(kw); reserved = kw.pop("reserved", 0)
            d = capi.exitance_desc(kw.pop("boundary", P.BOUNDARY_AABB), kw.pop("res", (4, 4)), **kw); d.reserved = reserved
            out = C.c_int32(-1)
            assert ctx.lib.mer_exitance_create(ctx.h, C.byref(d), C.byref(out)) != 0 and out.value == 0
            err = ctx.lib.mer_last_error(ctx.h).decode()
            assert err.startswith("mer_exitance_create: ") and re.search(msg, err), err
    finally:
        ctx.exitance_destroy(h); ctx.fluence_destroy(hf)


# ---- 14. the command line --------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("timed", [False, True])
def test_mer_render_exitance_writes_the_python_calls_map(ctx, tmp_path, timed):
    """mer_render --exitance=8,6 on the laser example: the float32 .npy [frames][faces][nv][nu][3] = sums / (paths x cell area [x binWidth]) of
    the map Context.exitance gives for the same scene and seed; --time-resolved takes the window from the film (tMin 4, tMax 9, tRes 0.5)"""
    scene = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
    defines = {"samples": "2", "tMin": "4", "tMax": "9", "tRes": "0.5", "medium": "homogeneous"}
    out = str(tmp_path / "exit.npy")
    args = [os.path.join(ROOT, "mitsubaer_amd", "mer_render"), "--exitance=8,6", "--accept-cos=0.25", "--seed", "3", "-o", out] + (["--time-resolved"] if timed else [])
    for k, v in defines.items():
        args += ["-D", "%s=%s" % (k, v)]
    r = subprocess.run(args + [scene], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "paths %d " % (128 * 96 * 2) in r.stdout and "ended 0" in r.stdout and "rejected" in r.stdout
    data = np.load(out)
    frames = 10 if timed else 1
    assert data.shape == (frames, 6, 6, 8, 3) and data.dtype == np.float32
    d, spp = host.flatten_xml(scene, defines)
    assert spp == 2 and d.integrator == P.INTEGRATOR_PTRACER and d.boundary == P.BOUNDARY_AABB
    kw = dict(frames=10, t_min=d.min_bound, t_bin=d.bin_width) if timed else {}
    sums, t = ctx.exitance(d, (8, 6), spp, cos_min=0.25, seed=3, **kw)
    assert t[0] == 128 * 96 * 2 and sums.sum() > 0 and t[11] > 0
    ext = np.array(d.bmax[:], np.float64) - np.array(d.bmin[:], np.float64)
    area = np.array([ext[(f // 2 + 1) % 3] * ext[(f // 2 + 2) % 3] / 48 for f in range(6)])
    want = sums / (t[0] * area[None, :, None, None, None] * (np.float64(d.bin_width) if timed else 1.0))
    np.testing.assert_allclose(data, want.astype(np.float32), rtol=1e-6, atol=0)
    got = [float(v) for v in re.search(r"rejected (\S+) (\S+) (\S+)", r.stdout).groups()]
    np.testing.assert_allclose(got, t[11:14], rtol=1e-6)
