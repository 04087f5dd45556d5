"""tests/transient64.py, the float64 references of tests/test_gpu_transient_extra.py, checked before they judge the HIP path: the
time-resolved volpath against the steady volpaths it restates, against ref64.point_single_scatter and against the single-scatter quadratures
(which must have converged); the calibrated shift; bounce orders; the CPU oracle where it knows the scene, at a bin width that resolves an
edge; and, for every scene of the GPU tests, the conditions that keep those tests honest -- enough tested cells, no hidden tail, a
non-trivial profile, and a wrong bookkeeping that the scene tells apart.  CPU only."""
import numpy as np
import pytest
from mitsubaer_amd import params as P
from tests import ref64, scenes, sensors64 as S, transient64 as T, volpath64_all as va, volpath64_multi as vm, volpath64_shapes as vs, volpath64_spot as vsp
from tests.envmap64 import EnvMap64, sun_and_gradient, rot

CAM = np.asarray(P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0]), np.float64)
PENCIL = np.asarray(P.look_at([-3, 0, 0], [-2, 0, 0], [0, 1, 0]), np.float64)
MED = (1.0, 0.5, 0.5)                                                           # sigma_s, sigma_a, g
RECT = np.array([[0, 0, -1, -1.5], [0, 0.15, 0, 0.4], [0.15, 0, 0, 0.1]], np.float64)
RECT_ABOVE = np.array([[1.5, 0, 0, 0], [0, 0, -1, 2.5], [0, -1.5, 0, 0]], np.float64)
SPOT = np.array([[1.0, 0, 0, 0.3], [0, 0, -1, 0.6], [0, 1, 0, -0.2]])
ALL = (0.0, 1.0, 1000)                                                          # frames that drop nothing


def _z(a, va_, b, vb=0.0):
    return (a - b) / np.sqrt(va_ + vb + 1e-20)


# ---- 1. the walk is the steady volpaths', and its frames add up

def test_frames_sum_to_the_steady_film_which_is_volpath64_all():
    """every feature at once on a thin lens: on the same seed the walk draws what tests/volpath64_all.py draws, so the steady film is its film to
    round-off, and the frames of a film that drops nothing sum to it to 1e-12 -- transient, calibrated and bounce alike"""
    env = lambda: EnvMap64(sun_and_gradient(8, 16), rot([0.3, 1.0, -0.4], 57.0), 0.5)
    scene = lambda rects: dict(kind=S.THINLENS, points=[([0.2, 0.3, -0.1], 3.0)], spots=[vsp.Spot(SPOT, 5.0, 60.0)], env=env(), sigma_s=MED[0], sigma_a=MED[1], g=MED[2],
                               width=8, height=8, fov_x_deg=50.0, cam_to_world=CAM, aperture_radius=0.3, focus_distance=3.0, spp=64, seed=3, **rects)
    rects = [vm.Rect(RECT_ABOVE, 3.0), vm.Rect(RECT, 4.0)]
    films = T.render(films=[T.Spec(ALL), T.Spec((-500.0, 1.0, 1000), calibrated=True), T.Spec(ALL, "bounce")], **scene(dict(shapes=rects)))
    ref = va.render(**scene(dict(rects=rects)))[0][..., 0]
    for f in films:
        assert f.steady.min() > 0
        np.testing.assert_allclose(f.steady, ref, rtol=1e-9)
        np.testing.assert_allclose(f.pix, f.steady, rtol=1e-12)
        np.testing.assert_allclose(f.tot.sum(), f.steady.sum(), rtol=1e-12)
        np.testing.assert_allclose(f.mean.sum(1), f.steady.reshape(2, 4, 2, 4).sum((1, 3)).ravel(), rtol=1e-12)
    assert (films[0].tot > 0).sum() > 4 and (films[2].tot > 0).sum() > 4


def test_the_steady_film_of_the_shapes_is_volpath64_shapes():
    m = vs.MIXED
    cam = np.asarray(P.look_at(*vs.MIXED_CAM), np.float64)
    f = T.render(S.PERSPECTIVE, [], [], vs.mixed_shapes(), m["env"], m["sigma_s"], m["sigma_a"], m["g"], 8, 8, m["fov_x_deg"], cam, spp=64, seed=5, frames=ALL)
    ref = vs.render(vs.mixed_shapes(), m["env"], m["sigma_s"], m["sigma_a"], m["g"], 8, 8, m["fov_x_deg"], cam, spp=64, seed=5)[0]
    np.testing.assert_allclose(f.steady, ref, rtol=1e-9)
    np.testing.assert_allclose(f.pix, f.steady, rtol=1e-12)


# ---- 2. single scattering: the point emitter's closed form and the new quadratures

def test_one_point_emitter_reproduces_point_single_scatter():
    """max_depth 3, a point inside the cube, isotropic: ref64.point_single_scatter's integrand binned by depth + distance; per frame within 4
    sigma of the volpath's own variance, and nothing where the closed form has nothing"""
    sa, ss = T.SINGLE_MEDIUM
    q = [0.1, 0.6, -0.2]
    f = T.render(S.PERSPECTIVE, [(q, 1.0)], [], [], 0.0, ss, sa, 0.0, 2, 2, 0.02, PENCIL, spp=20000, seed=2, chunk=4096, frames=T.SINGLE_FRAMES, max_depth=3, hide_emitters=True)
    _, t, w, r = ref64.point_single_scatter(T.PENCIL_O, T.PENCIL_D, 2.0, 4.0, sa, ss, q, n=400000)
    ref = 4 * T._bin(t + r, w, T.SINGLE_FRAMES)                                 # a cell sums its 4 pixels
    z = _z(f.tot, f.tot_var, ref)
    print("point: max |z| %.2f over %d frames, totals %.5f vs %.5f" % (np.abs(z).max(), (ref > 0).sum(), f.tot.sum(), ref.sum()))
    assert (ref > 0).sum() >= 8 and np.all(np.abs(z) <= 4) and np.all(f.tot[ref == 0] == 0)


@pytest.fixture(scope="module")
def profiles():
    """name -> (the refined quadrature over SINGLE_FRAMES, its changes on halving the step: transient64.refined)"""
    return {n: T.refined(lambda **kw: T.single_case(n)["profile"](T.SINGLE_FRAMES, **kw), **T.single_case(n)["steps"]) for n in T.SINGLE_NAMES}


@pytest.mark.parametrize("name", T.SINGLE_NAMES)
def test_quadrature_has_converged(profiles, name):
    """on halving the step every frame total that holds at least 1 % of the largest one changes by less than 1e-3 of itself; a fainter frame,
    which the support's edge grazes, by less than 1e-3 of that 1 % (1e-5 of the largest frame)"""
    prof, change, faint = profiles[name]
    print("%s: frame totals change by %.2e (faint frames: %.2e of 1 %% of the largest) on halving the step; %d frames lit" % (name, change, faint, (prof > 0).sum()))
    assert change < 1e-3 and faint < 1e-3
    assert (prof > 0.02 * prof.sum()).sum() >= 6                                  # a profile, not a spike


@pytest.mark.parametrize("name", T.SINGLE_NAMES)
def test_one_emitter_reproduces_its_quadrature(profiles, name):
    prof = 4 * profiles[name][0]
    f = T.single_render(name, 20000, seed=4)
    z = T.profile_z(f.tot, f.tot_cov, prof)                                       # frames the support merely grazes are pooled with the next
    print("%s: max |z| %.2f over %d pools, totals %.5f vs %.5f" % (name, np.abs(z).max(), len(z), f.tot.sum(), prof.sum()))
    assert len(z) >= 6 and len(z) >= 0.75 * T.resolved_frames(prof)              # pooling only gathers the grazed frames
    assert np.all(np.abs(z) <= 4) and np.all(f.tot[prof == 0] == 0)
    assert abs(f.tot.sum() - prof.sum()) <= 4 * np.sqrt(f.tot_cov.sum())


def test_calibrated_is_the_profile_shifted_by_the_camera_edge():
    """the pencil camera's edge is 2 = 8 frames of 0.25: on one walk the calibrated film over [2, 10) is frames 8 ... 39 of the plain one"""
    lo, bw, F = T.SINGLE_FRAMES
    for name in ("spot", "sphere"):
        c = T.single_case(name)
        a, b = T.single_render(name, 4000, seed=6, films=[T.Spec((lo, bw, F + 8), max_depth=c["max_depth"]), T.Spec(T.SINGLE_FRAMES, calibrated=True, max_depth=c["max_depth"])])
        assert b.tot.sum() > 0 and b.tot[:8].sum() > 0
        np.testing.assert_allclose(b.tot, a.tot[8:], rtol=1e-12, atol=0)
        prof = c["profile"]((lo, bw, F + 8), **c["steps"]); cal = c["profile"](T.SINGLE_FRAMES, True, **c["steps"])
        np.testing.assert_allclose(cal, prof[8:], rtol=1e-9, atol=1e-15)
        w = T.single_render(name, 4000, seed=6, calibrated=True, wrong="calibrated_ignored")
        np.testing.assert_allclose(w.tot, a.tot[:F], rtol=1e-12)


def test_bounce_frame_k_holds_one_scattering_order():
    """emitters outside the cube only: raising max_depth by one populates exactly one more frame and leaves the others as they were"""
    args = dict(kind=S.PERSPECTIVE, points=[], spots=[], shapes=[vm.Rect(RECT_ABOVE, 3.0)], env=0.2, sigma_s=MED[0], sigma_a=MED[1], g=MED[2], width=8, height=8,
                fov_x_deg=90.0, cam_to_world=CAM, spp=64, seed=7)                  # wide: some rays see the sky, some the rectangle's underside
    f = T.render(films=[T.Spec(T.BOUNCE_FRAMES, "bounce", max_depth=d) for d in (5, 6, 7)], **args)
    for i, d in enumerate((5, 6, 7)):
        lit = f[i].tot > 0
        assert np.array_equal(lit, np.arange(16) < d), (d, lit)                  # frames 0 (the sky), 1 (the rectangle), 2 (unscattered) ... d - 1
        if i:
            assert np.array_equal(f[i].mean[:, :d - 1], f[i - 1].mean[:, :d - 1])
    w = T.render(mode="bounce", frames=T.BOUNCE_FRAMES, max_depth=6, wrong="bounce_counts_exit", **args)
    assert np.array_equal(w.tot[:3], f[1].tot[:3]) and w.tot[3] == 0 and np.allclose(w.tot[4:7], f[1].tot[3:6], rtol=1e-12)


# ---- 3. the oracle, where it knows the scene, at a bin width that resolves an edge

@pytest.mark.parametrize("name", ["point", "rectangle"])
def test_oracle_transient_matches_float64_at_a_quarter_unit(orc, name):
    """one point emitter / one rectangle, homogeneous, pinhole, [0, 16) in 64 frames: the oracle's frame totals (8 seeds of 1024 samples, the
    variance from the seeds) against the float64 frame totals, every tested frame within 4 sigma.  Frames are tested and pooled by the rule of
    the cells (transient64.tested_cells, the whole image as one block): a tail frame that a handful of paths reach has no usable variance"""
    kw = dict(w=16, h=16, fov_x_deg=50.0, cam_to_world=P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0]), sigma_s=[MED[0]] * 3, sigma_a=[MED[1]] * 3, phase=P.PHASE_HG, g=MED[2],
              env_radiance=[0.0] * 3, max_depth=-1, rr_depth=1 << 20, rfilter=P.FILTER_BOX, rfilter_param=0.5, decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=0.0, max_bound=16.0, bin_width=0.25)
    if name == "point":
        p = scenes.homogeneous_scene(point_position=[0.2, 0.3, -0.1], point_intensity=[3.0] * 3, **kw)
        ref = dict(points=[([0.2, 0.3, -0.1], 3.0)], shapes=[])
    else:
        p = scenes.homogeneous_scene(area_to_world=RECT_ABOVE, area_radiance=[3.0] * 3, **kw)
        ref = dict(points=[], shapes=[vm.Rect(RECT_ABOVE, 3.0)])
    f = T.render(S.PERSPECTIVE, ref["points"], [], ref["shapes"], 0.0, *MED, 16, 16, 50.0, CAM, spp=1024, seed=1, frames=(0.0, 0.25, 64))
    tot = []
    for seed in range(8):
        film = orc.render(p, 0, 1024, 100 + seed)[0]
        tot.append((film[..., :-2].reshape(16, 16, 64, 3)[..., 0].astype(np.float64) / film[..., -1:]).sum((0, 1)))
    tot = np.stack(tot)
    whole = T.Film(mean=f.tot[None], cov=f.tot_cov[None])
    groups, untested = T.tested_cells(whole)
    z = np.array([_z(tot[:, a:b].sum(1).mean(), tot[:, a:b].sum(1).var(ddof=1) / 8, *T._group(whole, 0, a, b)) for _, a, b in groups])
    print("%s: max |z| %.2f over %d tested frames (untested %.4f); totals %.4f (oracle) %.4f (float64); tail %.4f" % (name, np.abs(z).max(), len(z), untested, tot.mean(0).sum(), f.tot.sum(), f.tail))
    assert len(z) >= 8 and untested <= 0.02 and f.tail < 0.01
    assert np.all(np.abs(z) <= 4), z


# ---- 4. the scenes of the GPU tests: honest conditions, and wrong references that the scenes tell apart

def _honest(ref, least):
    groups, untested = T.tested_cells(ref)
    pools, untested_totals = T.tested_frames(ref)
    print("   %d tested cells of %d (%d frame totals), untested share %.4f (%.4f), tail %.4f, %d non-trivial frames"
          % (len(groups), ref.mean.size, len(pools), untested, untested_totals, ref.tail, T.nontrivial_frames(ref)))
    assert untested <= 0.02 and untested_totals <= 0.02 and ref.tail <= 0.01 and T.nontrivial_frames(ref) >= least
    return T.tested(ref)


@pytest.mark.parametrize("name", T.MULTI_NAMES)
def test_multi_scene_references_are_honest_and_tell_the_wrong_rules_apart(name):
    """per scene: the tested cells leave at most 2 % of the film untested, at most 1 % of the energy lies outside the bounds, at least 8 (4 for
    the bounce film) frames hold more than 2 % each -- and the film of every applicable wrong rule disagrees with the right one under the very
    rule the GPU film must pass"""
    R = T.multi_reference(name)
    g = _honest(R["transient"], 8)
    assert not T.agrees(R["transient/edge_from_exit"], R["transient"], g)
    g = _honest(R["bounce"], 4)
    assert not T.agrees(R["bounce/bounce_counts_exit"], R["bounce"], g)
    if name in T.LENS_NAMES:
        g = _honest(R["calibrated"], 8)
        assert not T.agrees(R["transient"], R["calibrated"], g)                   # "calibrated_ignored" is the plain transient film
    if name in T.MODULATED_NAMES:
        for what in ("sine", "square"):
            assert np.isfinite(R[what].pix).all() and np.abs(R[what].pix).sum() > 0.1 * R["transient"].pix.sum()
        assert not T.agrees_per_pixel(R["sine"], R["square"])[0]


def test_two_seeds_of_the_right_reference_agree():
    """the rule does not reject the reference itself: two independent walks of one scene"""
    p, args = T.multi_scene("mixed_shapes")
    a = T.multi_reference("mixed_shapes")["transient"]
    b = T.render(frames=T.TRANSIENT_FRAMES, spp=T.MULTI_SPP, seed=2, **args)
    assert T.agrees(b, a, T.tested(a))
