"""Where K_replay (replay_kernel, mer_sensitivity.hpp) puts its deposits.  Its second pass is a hand copy of K_fluence_track's wave-uniform
skeleton -- the curved stepping loop, TrackDDA's cutting, the run of chords and its flush -- and tests/test_gpu_sensitivity.py holds most
cases only to sums (cells + dropped = w x length, sum(J) = -dW / d sigma_a, detected weight = the exitance window).  A wrong cell on a
curved ray, a run flushed into the previous cell, a piece attributed across a null collision or an off-by-one at a face keep those sums.

1. "Every path is detected": in a non-absorbing medium with the roulette out of reach and a spherical boundary whose one face is the
   detector's window, every path is detected with w = T power, T = 1 up to float32 rounding, and the track-length grid deposits T power l
   for the same pieces cut the same way: J equals mer_fluence_track's grid cell by cell, deterministically, in all 14 instantiations.
2. Against tests/sensitivity64.py where the GPU had never been compared: the sigma_t ramp (null collisions), the albedo grid, `maximum`
   and `single` with medium_sampling_weight 0.7, rif_const 1.33 under a gate; per cell and per slab.
3. Curved rays: the length a bending beam leaves in every cell against a float64 trace of the exact ray.

Measured on the MI355X: in each test's docstring and in DESIGN.md, "What pins K_replay"."""
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, synth
from tests import scenes
from tests import test_sensitivity64 as T
from tests import test_lightpath64 as L
from tests import test_gpu_exitance as TE
from tests import test_gpu_fluence as TG
from tests import test_gpu_lightpath_media as TM
from tests import test_gpu_lightpath_parent as TPAR
from tests import test_gpu_ptracer as TP
from tests import test_gpu_sensitivity as TS
from tests.fluence_track64 import _pieces

pytestmark = pytest.mark.gpu
W = H = TS.W
RTOL_PIECE = TS.RTOL_PIECE
RAGGED = ((5, 4, 3), ((-0.6, -0.5, -0.7), (0.5, 0.7, 0.4)))          # its own box, which cuts the sphere and the cube; no face at a round number
ONE_CELL = ((1, 1, 1), RAGGED[1])
POINT_O = [0.1, -0.2, 0.3]

# ---- 1. every path is detected: J is the track-length grid -------------------------------------------------------------------------------

_H = TPAR._H
_BSPLINE = dict(rif_mode=P.RIF_BSPLINE3, rif_aabb=([-1.6] * 3, [1.6] * 3))          # TPAR.SCENES["bspline"]: the cube lies inside the spline's limits
RAYS = {
    "straight": lambda: {},
    "trilinear Verlet": lambda: dict(rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=_H, stepper=P.STEP_VERLET),
    "trilinear RK4": lambda: dict(rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=_H, stepper=P.STEP_RK4),
    "B-spline Verlet": lambda: dict(rif=synth.radial_rif(16, (-1.6,) * 3, (1.6,) * 3), stepsize=_H, stepper=P.STEP_VERLET, **_BSPLINE),
    "B-spline RK4": lambda: dict(rif=synth.radial_rif(16, (-1.6,) * 3, (1.6,) * 3), stepsize=_H, stepper=P.STEP_RK4, **_BSPLINE),
    "acoustic Verlet": lambda: dict(stepsize=_H, stepper=P.STEP_VERLET, **TPAR._AC),
    "acoustic RK4": lambda: dict(stepsize=_H, stepper=P.STEP_RK4, **TPAR._AC),
}
NO_LOSS = dict(rr_depth=T.DERIV["rr_depth"], max_depth=-1)


def _ramp_density():
    """the ramp's 2 x 2 x 2 grid: 0.125 on the z = -1 nodes, 1 on the z = +1 nodes; with density_scale 1, sigma_t <= 1"""
    d = np.full((2, 2, 2), 0.125, np.float32); d[1] = 1.0
    return d


MEDIA = {
    "homogeneous": lambda **kw: TE._base(sigma_s=[0.5] * 3, sigma_a=[0.0] * 3, **NO_LOSS, **kw),
    "gridded sigma_t": lambda **kw: TE._grid(density=_ramp_density(), density_scale=1.0, albedo=[1.0] * 3, **NO_LOSS, **kw),
}
EMITTERS = {"point inside": lambda: P.point_emitter(POINT_O, [TE.INTENSITY] * 3), "beam from outside": lambda: TS._beam()}


def _both(ctx, p, faces, spp, seed, res, box):
    """the sensitivity render of every detector `faces` (each the whole raster of its face, no cone, no gate), summed, and the track-length
    render of the same scene, shard, seed and box: ((J, totals, counters of the last detect pass, detected per face), (sums, totals, counters))"""
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    hk = ctx.fluence_track_create(res, box[0], box[1])
    try:
        ctx.counters_reset()
        ctx.render_fluence(sc, hk, 0, spp, seed=seed)
        cnt_k = [int(v) for v in ctx.counters()]
        ks, kt = ctx.fluence_read(hk)
        js, jt, per_face = 0.0, 0.0, []
        for face in faces:
            h = ctx.sensitivity_create(res, box[0], box[1], capi.detector_desc(sc.boundary, (4, 4), face))
            try:
                ctx.counters_reset()
                ctx.render_sensitivity(sc, h, 0, spp, seed=seed)
                cnt_j = [int(v) for v in ctx.counters()]
                s, t = ctx.sensitivity_read(h)
            finally:
                ctx.sensitivity_destroy(h)
            assert cnt_j == cnt_k, "the detect pass walks the track render's paths"
            assert t[0] == W * H * spp and t[12] == 0 and t[7] == 0 and not t[13:].any()
            js = js + s; jt = jt + t; per_face.append(t[8])
    finally:
        ctx.fluence_destroy(hk)
        for v in vols:
            v.destroy()
    assert np.isfinite(js).all() and np.isfinite(ks).all()
    return (js, jt, cnt_j, per_face), (ks, kt, cnt_k)


def _same_as_the_track_grid(j, k, paths, what, n_faces=1):
    """J against the track-length grid: cell by cell, channel by channel, the dropped totals, and the same cells filled"""
    (js, jt, cnt, per_face), (ks, kt, _) = j, k
    assert jt[8] == paths and jt[0] == n_faces * paths and kt[0] == paths
    assert jt[12] == 0 and jt[7] == 0 and kt[7] == 0
    assert np.array_equal(js != 0, ks != 0), "a cell filled in one grid and empty in the other"
    assert (ks != 0).any()
    rel = np.abs(js - ks)[ks != 0] / ks[ks != 0]
    print("%s: %d of %d values filled, largest relative difference of a cell %.2e, of dropped %.2e; dropped / (cells + dropped) %.3f; events per path %.2f"
          % (what, (ks != 0).sum(), ks.size, rel.max(), (np.abs(jt[4:7] - kt[4:7]) / kt[4:7]).max(), kt[4] / (ks[..., 0].sum() + kt[4]), cnt[capi.C_REAL] / paths))
    np.testing.assert_allclose(js, ks, rtol=RTOL_PIECE, atol=0)
    np.testing.assert_allclose(jt[4:7], kt[4:7], rtol=RTOL_PIECE, atol=0)
    return per_face


@pytest.mark.parametrize("emitter", list(EMITTERS))
@pytest.mark.parametrize("medium", list(MEDIA))
@pytest.mark.parametrize("rays", list(RAYS))
def test_every_path_detected_is_the_track_length_grid(ctx, rays, medium, emitter):
    """The unit sphere, sigma_a = 0 (homogeneous sigma_s = 0.5, or a gridded sigma_t <= 1 with albedo 1: delta tracking with null
    collisions), rr_depth out of reach, max_depth -1, the detector the sphere's whole raster: 16 x 16 x 4 = 1024 paths into the ragged
    5 x 4 x 3 grid, whose box cuts the sphere (dropped > 0), and into one cell.  J == the track-length grid within RTOL_PIECE per cell and
    channel and for the dropped totals, the same cells filled, counters equal entry for entry, every path detected, none ended, no replay
    disagreement.  The beam's exterior leg deposits nothing in either.

    Why 1e-5 suffices: the homogeneous collision factor (sigma_s tr) / (sigma_t tr) is exactly 1, the gridded one albedo sigma (1 / sigma)
    within an ulp or two per event, and a cell's sum is dominated by paths of a few events.

    Measured on the MI355X, largest relative difference of a cell (point, beam; homogeneous then gridded): straight 2.2e-8, 3.0e-8; 1.3e-8,
    5.6e-8.  Trilinear Verlet 5.9e-8, 1.0e-7; 4.6e-8, 1.6e-7.  Trilinear RK4 4.7e-8, 1.3e-7; 4.0e-8, 1.2e-7.  B-spline Verlet 4.7e-8, 1.0e-7;
    6.2e-8, 8.7e-8.  B-spline RK4 4.4e-8, 1.3e-7; 7.7e-8, 7.7e-8.  Acoustic Verlet 7.7e-8, 9.7e-8; 4.2e-8, 9.1e-8.  Acoustic RK4 4.3e-8,
    1.9e-7; 8.8e-8, 1.3e-7.  Dropped totals: at most 2.9e-8.  0.5 - 1.0 real collisions per path; 38 - 48 % of the length is dropped.
    A replay whose curved run restarts without flushing turns the 24 curved cases red, one whose straight deposit goes to the previous
    trip's cell the 4 straight ones (mutated builds, run once, never committed)."""
    spp, seed = 4, 11
    paths = W * H * spp
    p = MEDIA[medium](emitters=[EMITTERS[emitter]()], **TE._sphere(), **RAYS[rays]())
    for res, box in (RAGGED, ONE_CELL):
        j, k = _both(ctx, p, (0,), spp, seed, res, box)
        _same_as_the_track_grid(j, k, paths, "%s, %s, %s, %s" % (rays, medium, emitter, "x".join(map(str, res))))
        assert np.all(k[1][4:7] > 0)                                     # the box cuts the sphere
        if emitter == "point inside":
            assert k[0][..., 0].sum() + k[1][4] > 0.5 * paths * 4 * np.pi * TE.INTENSITY     # a path flies at least the 0.6 to the sphere
    if medium == "gridded sigma_t":
        assert j[2][capi.C_TENTATIVE] > 1.2 * j[2][capi.C_REAL] > 0      # null collisions happened


@pytest.mark.parametrize("rays", ["straight", "trilinear Verlet"])
def test_six_faces_of_the_cube_sum_to_the_track_length_grid(ctx, rays):
    """the cube, homogeneous sigma_s = 0.5: six detectors, faces 0 ... 5, each the whole raster of its face.  Their sum is the track-length
    grid under the asserts of test_every_path_detected_is_the_track_length_grid, and the detected paths sum to the paths: no exit belongs to
    two faces or to none.  Measured on the MI355X: largest relative difference of a cell 2.9e-8 and 6.3e-8 (straight; point, beam), 8.6e-8 and
    1.6e-7 (trilinear Verlet); detected per face 117 ... 235 (point), 55 ... 612 (beam, face 5)"""
    spp, seed = 4, 13
    paths = W * H * spp
    for emitter in EMITTERS:
        p = MEDIA["homogeneous"](emitters=[EMITTERS[emitter]()], **RAYS[rays]())
        j, k = _both(ctx, p, range(6), spp, seed, *RAGGED)
        per_face = _same_as_the_track_grid(j, k, paths, "cube, %s, %s" % (rays, emitter), n_faces=6)
        print("detected per face", per_face)
        assert sum(per_face) == paths and (emitter != "point inside" or min(per_face) > 0)


# ---- 2. against the float64 restatement --------------------------------------------------------------------------------------------------

K, SPP = T.K, TG.SPP
assert W * H * SPP == T.CASE_PATHS
_STRATEGY = {"maximum": P.STRATEGY_MAXIMUM, "single": P.STRATEGY_SINGLE}


def _case_scene(name):
    """the scene of tests/test_sensitivity64.py's CASES[name], and its detector"""
    c = T.CASES[name]
    em = TM.BEAM if c["emitter"] == "beam" else P.point_emitter(list(T.POINT_O), list(T.POINT_I))
    m = c["medium"]
    if m[0] == "ramp":
        p = TM._ramp(emitters=[em], **({} if m[1] is None else dict(albedo_mode=P.ALBEDO_GRID, albedo_grid=scenes.rgb_albedo(8))))
    else:
        ch = L.CHROMA[m[1]]
        p = TG._base(sigma_s=list(ch["sigma_s"]), sigma_a=list(ch["sigma_a"]), g=L.G, strategy=_STRATEGY[m[0]], medium_sampling_weight=m[2],
                     rif_const=c.get("n", 1.0), emitters=[em])
    return p, dict(face=c["face"], window=T.WHOLE, cos_min=c.get("cos_min", 0.0), t_min=c.get("t_min", 0.0), t_bin=c.get("t_bin", 0.0))


@pytest.mark.parametrize("name", list(T.CASES))
def test_matches_float64(ctx, name):
    """K = 16 batches of 16 x 16 x 64 = 16 384 paths, seeds s0 + j, the dense layout, a 4^3 grid over the cube, a 4 x 4 raster, against
    tests/sensitivity64.py (test_sensitivity64.check_case): every cell the reference fills under the bar; totals[1..3], [8], [9..11]
    within 4 sigma; the 3 x 4 x 3 slab profiles (J summed over each plane normal to x, y, z: thousands of paths per batch, percent-level
    power where a cell's mean has a relative sd of 5 - 15 %) within 4 sigma; totals[12] == totals[7] == 0; in the ramp, null collisions.

    `maximum` keeps the strong chroma: reference against reference, three pairs of seeds put 0 of 156 - 162 compared cells beyond 4 sigma
    (max z 3.06, 2.46, 2.57; totals z <= 2.82; slabs z <= 3.08) -- the medium chroma, which the time grid had to take, is not needed.
    With the gate [0.5, 3.5) at n = 1.33 the slab farthest from the detector is dark: 156 of 192 cells are compared there, every cell elsewhere
    but in "ramp, forward" (189: one corner cell is empty in the reference's seed).

    Reference against reference, measured on the CPU (compared cells, beyond 4 sigma, max z, largest total z, largest slab z):
      ramp, forward 189, 0, 2.93, 0.63, 2.27;  ramp, back-scatter 192, 0, 3.02, 0.94, 1.66;  ramp, side, cone and gate 192, 0, 2.29, 1.06, 1.74;
      ramp with albedo grid 192, 0, 2.11, 1.01, 1.45;  maximum 156, 0, 3.06, 2.82, 3.08;  single 192, 0, 2.52, 2.99, 3.23.
    The GPU against the reference, measured on the MI355X (the same five figures):
      ramp, forward 189, 0, 2.82, 1.59, 1.68;  ramp, back-scatter 192, 0, 2.48, 1.30, 2.26;  ramp, side, cone and gate 192, 0, 2.96, 0.95, 1.67;
      ramp with albedo grid 192, 0, 2.28, 1.46, 2.14;  maximum 156, 0, 2.38, 1.70, 2.31;  single 192, 0, 2.74, 0.76, 1.04.
    Tentative / real collisions in the ramp: 2.03.  The reference's relative sd of the mean: per cell median 0.05 ... 0.16, per slab 0.009 ... 0.017."""
    p, dk = _case_scene(name)
    ref, rt = T.case_ref(name)
    ctx.counters_reset()
    got = [TS._render(ctx, p, dk, SPP, seed=3000 + 100 * list(T.CASES).index(name) + b) for b in range(K)]
    cnt = ctx.counters()
    s = np.array([g[0] for g in got]); t = np.array([g[1] for g in got])
    assert not t[:, 4:7].any()
    res = T.check_case(s, t, ref, rt, "GPU " + name)
    print("GPU %s: compared cells, beyond 4 sigma, max z, largest total z, largest slab z: %s; tentative %d, real %d" % (name, res, cnt[capi.C_TENTATIVE], cnt[capi.C_REAL]))
    if name.startswith("ramp"):
        assert cnt[capi.C_TENTATIVE] > 1.5 * cnt[capi.C_REAL] > 0


# ---- 3. curved rays: where the beam's length lands ---------------------------------------------------------------------------------------

CURVED_RES = (8, 8, 8)


CURVED_BEAMS = {"y = -0.5": TE.CURVED_O, "y = -0.6": [0.25, -0.6, -3.0]}


def _curved_lengths(o, h=0.002):
    """the beam from `o` through n = RIF_A + RIF_B y in float64 (RK4 in arc length, TE._curved_trace's steps; the last one shortened
    by bisection): the arc length inside every cell of the 8^3 grid over the cube (each step's chord cut at the grid's planes), and the
    cell that holds the exit"""
    p = np.array([o[0], o[1], -1.0]); v = np.array(TE.BEAM_D) * (TP.RIF_A + TP.RIF_B * p[1])
    pts, hs = [p], []
    for _ in range(100000):
        q, w = TP._rk4(p, v, h)
        if np.all(np.abs(q) <= 1):
            pts.append(q); hs.append(h); p, v = q, w
            continue
        lo, hi = 0.0, h
        for _ in range(60):
            mid = 0.5 * (lo + hi)
            if np.all(np.abs(TP._rk4(p, v, mid)[0]) <= 1):
                lo = mid
            else:
                hi = mid
        pts.append(TP._rk4(p, v, lo)[0]); hs.append(lo)
        break
    else:
        raise AssertionError("the beam never left the cube")
    pts, hs = np.array(pts), np.array(hs)
    x, d = pts[:-1], pts[1:] - pts[:-1]
    chord = np.linalg.norm(d, axis=1)
    keep = chord > 0
    x, d, chord, hs = x[keep], d[keep] / chord[keep, None], chord[keep], hs[keep]
    a, b, idx, inside = _pieces(x, d, chord, CURVED_RES, (-1, -1, -1), (1, 1, 1))
    ell = np.zeros(int(np.prod(CURVED_RES)))
    np.add.at(ell, idx[inside], ((b - a) * (hs / chord)[:, None])[inside])          # a chord's pieces share the step's arc length
    assert abs(ell.sum() - hs.sum()) < 1e-9
    ie = np.minimum(np.floor((pts[-1] + 1) / 2 * np.array(CURVED_RES)).astype(int), np.array(CURVED_RES) - 1)
    return ell.reshape(CURVED_RES[::-1]), (ie[2], ie[1], ie[0]), pts[-1]


@pytest.mark.parametrize("beam", list(CURVED_BEAMS))
@pytest.mark.parametrize("stepper", [P.STEP_VERLET, P.STEP_RK4])
def test_curved_beam_leaves_its_length_in_the_cells_of_the_exact_ray(ctx, stepper, beam):
    """The clear cube with n = 1.3 + 0.15 y (exact under trilinear interpolation), a beam along +z that bends towards +y, the detector face 5 with its whole raster: every path is detected with w = P, so J_c / (paths P) is the geometric length of the one ray in
    cell c of the 8^3 grid.  Stepsize h = 0.0125.  Against the float64 trace: |l_gpu - l_ref| <= 2 h in every cell but the exit's, where
    -3.5 h <= l_gpu - l_ref <= 2 h (the last piece before the boundary, up to 1.5 h, deposits nothing: mer_fluence_track.hpp).  2 h is the
    most by which two face crossings can move when the GPU's ray stays within h of the exact one -- a ceiling, not a fit: tests/closed_form.py
    holds RK4 to the exact ray of a linear index within 4e-6, and Verlet to 0.0303 h at the arc length 0.6 with this slope; growing with
    the square of the arc length to this beam's 2.1 that is 0.37 h.  Cells the exact ray does not touch and that share no face with a
    touched one are exactly 0; the cells sum to totals[9..11] / (paths P) within RTOL_PIECE.

    Two beams: from TE.CURVED_O, which starts on the plane y = -0.5 between two rows of cells and leaves at y = -0.254, just short of the next
    plane -- one column of 8 cells, 0.004 from a second one; and from y = -0.6, which crosses the plane y = -0.5 half-way and leaves 9 cells lit.

    Measured on the MI355X, (l_gpu - l_ref) / h: every cell but the exit's -0.004 ... 0.001 (Verlet), -0.001 ... 0.001 (RK4); the exit cell
    -0.52 in all four cases; sum of l_gpu 2.0134 ... 2.0141 against 2.0201 and 2.0206."""
    h, spp = 0.0125, 4
    paths = W * H * spp
    ell, exit_cell, xe = _curved_lengths(CURVED_BEAMS[beam])
    touched = ell > 0
    assert touched.sum() >= 8 and (beam == "y = -0.5" or len(set(np.argwhere(touched)[:, 1])) == 2)          # the second beam crosses y-cells
    near = touched.copy()
    for ax in range(3):
        for sh in (1, -1):
            r = np.roll(touched, sh, ax)
            edge = [slice(None)] * 3; edge[ax] = 0 if sh == 1 else -1
            r[tuple(edge)] = False
            near |= r
    p = TE._clear(rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=h, stepper=stepper, emitters=[TS._beam(CURVED_BEAMS[beam])])
    s, t = TS._render(ctx, p, dict(face=5, window=T.WHOLE), spp, res=CURVED_RES, seed=9)
    assert t[0] == t[8] == paths and t[12] == 0 and t[7] == 0 and not t[4:7].any()
    np.testing.assert_array_equal(t[1:4], paths * np.array(TS.POWER3))
    for c in range(3):
        lg = s[..., c] / (paths * TS.POWER3[c])
        diff = (lg - ell) / h
        assert np.all(lg[~near] == 0.0), "length in a cell away from the ray"
        rest = np.ones_like(touched); rest[exit_cell] = False
        if c == 0:
            print("stepper %d, beam %s: exit %s in cell %s; %d cells touched; (l_gpu - l_ref) / h: exit cell %.3f, other cells %.3f ... %.3f; sum of l_gpu %.5f, of l_ref %.5f"
                  % (stepper, beam, xe, exit_cell, touched.sum(), diff[exit_cell], diff[rest].min(), diff[rest].max(), lg.sum(), ell.sum()))
        assert np.all(np.abs(diff[rest]) <= 2.0), (diff[rest].min(), diff[rest].max())
        assert -3.5 <= diff[exit_cell] <= 2.0, diff[exit_cell]
        np.testing.assert_allclose(lg.sum(), t[9 + c] / (paths * TS.POWER3[c]), rtol=RTOL_PIECE, atol=0)
