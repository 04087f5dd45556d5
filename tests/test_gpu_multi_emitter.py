"""Several point and area emitters (mer_scene_desc.emitters): one emitter of each kind is selected per collision with probability
samplingWeight / sum (Scene::sampleAttenuatedEmitterDirect, src/librender/scene.cpp:854-898) from a forked stream, and its sample divided by
that probability.  Checked without an oracle: a one-entry list renders the single-emitter fields bit for bit; an emitter split into co-located
parts with power-of-two pdfs renders bit for bit what the whole one does; films are linear in the emitters; rectangles occlude each other."""
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi
from tests import scenes
from tests.test_oracle_kat import RECT_ABOVE

pytestmark = pytest.mark.gpu
RECT_BELOW = np.array([[1.0, 0, 0, 0.3], [0, 0, 1, -2.0], [0, 1.0, 0, 0]], np.float64)     # under the cube, facing up (+y)
PIN, POUT = [0.2, 0.3, -0.1], [-1.6, 1.4, 0.4]
I = [1.0, 0.5, 2.0]


def _paths(ctx, p, samples=(0, 1), seed=3):
    sc, vols = ctx.upload_scene(p)
    out = [ctx.render_paths(sc, s, seed=seed) for s in samples]
    for v in vols:
        v.destroy()
    return np.stack(out)


def _legacy_point(p, pos, inten=I):
    return p.copy(point_position=list(pos), point_intensity=list(inten))


def _curved(stepper, **kw):
    kw.setdefault("env_radiance", [0.3] * 3)
    return scenes.curved_scene(N=16, w=24, h=20, stepper=stepper, **kw)


def _rough(p):
    p.boundary_bsdf = P.BSDF_HROUGHDIELECTRIC; p.rough_distribution = P.MICROFACET_GGX; p.rough_alpha = 0.2; p.rough_sample_visible = 1
    return p


BASES = {
    "straight_point_in": (lambda: scenes.straight_scene(N=16, w=24, h=20), PIN),
    "straight_point_out": (lambda: scenes.homogeneous_scene(w=24, h=20, phase=P.PHASE_HG, g=0.5), POUT),
    "curved_verlet_point_in": (lambda: _curved(P.STEP_VERLET), PIN),
    "curved_rk4_point_out": (lambda: _curved(P.STEP_RK4), POUT),
    "curved_verlet_point_out": (lambda: _curved(P.STEP_VERLET, sigma_mode=P.SIGMA_HOMOGENEOUS), POUT),
    "rough_point_out": (lambda: _rough(scenes.homogeneous_scene(w=24, h=20, env_radiance=[0.2] * 3)), POUT),
}


@pytest.mark.parametrize("name", sorted(BASES))
def test_one_entry_list_equals_the_point_fields(ctx, name):
    make, pos = BASES[name]
    a = _paths(ctx, _legacy_point(make(), pos))
    b = _paths(ctx, make().copy(emitters=[P.point_emitter(pos, I, 2.5)]))
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(a, b)


@pytest.mark.parametrize("name", ["straight", "sphere"])
def test_one_entry_list_equals_the_area_fields(ctx, name):
    kw = dict(boundary=P.BOUNDARY_SPHERE, sph_radius=0.9) if name == "sphere" else {}
    base = scenes.straight_scene(N=16, w=24, h=20, **kw)
    a = _paths(ctx, base.copy(area_to_world=RECT_ABOVE, area_radiance=[3.0, 2.0, 1.0]))
    b = _paths(ctx, base.copy(emitters=[P.area_emitter(RECT_ABOVE, [3.0, 2.0, 1.0], 0.7)]))
    assert a.max() > 0 and np.array_equal(a, b)


@pytest.mark.parametrize("name", sorted(BASES))
def test_split_emitter_is_bit_exact(ctx, name):
    """one point of intensity I against co-located parts I/2 + I/2 (weights 1:1) and I/4 + 3I/4 (weights 1:3): every selection returns
    part / pdf = I exactly, and the selection draw comes from a forked stream, so every path is the same"""
    make, pos = BASES[name]
    whole = _paths(ctx, make().copy(emitters=[P.point_emitter(pos, I)]))
    half = _paths(ctx, make().copy(emitters=[P.point_emitter(pos, np.multiply(I, 0.5)), P.point_emitter(pos, np.multiply(I, 0.5))]))
    quarters = _paths(ctx, make().copy(emitters=[P.point_emitter(pos, np.multiply(I, 0.25), 1.0), P.point_emitter(pos, np.multiply(I, 0.75), 3.0)]))
    assert whole.max() > 0
    assert np.array_equal(whole, half)
    assert np.array_equal(whole, quarters)


def _block_stats(x, b=4):
    """x: [K samples, H, W, 3] -> per-(b x b block, channel) mean and standard error of the mean"""
    K, H, W, _ = x.shape
    y = x[:, :H // b * b, :W // b * b].reshape(K, H // b, b, W // b, b, 3).transpose(1, 3, 0, 2, 4, 5).reshape(H // b, W // b, -1, 3).astype(np.float64)
    return y.mean(2), y.std(2) / np.sqrt(y.shape[2])


def _linear(ctx, base, ea, eb, K=32):
    s = range(K)
    ab = _block_stats(_paths(ctx, base.copy(emitters=[ea, eb]), s, seed=11))
    a = _block_stats(_paths(ctx, base.copy(emitters=[ea]), s, seed=12))
    b = _block_stats(_paths(ctx, base.copy(emitters=[eb]), s, seed=13))
    diff = ab[0] - (a[0] + b[0])
    sig = np.sqrt(ab[1] ** 2 + a[1] ** 2 + b[1] ** 2)
    assert a[0].sum() > 0 and b[0].sum() > 0
    assert (np.abs(diff) <= 4 * sig + 1e-7).mean() > 0.99, np.abs(diff / np.maximum(sig, 1e-12)).max()
    tot = diff.sum(); tsig = np.sqrt((sig ** 2).sum())
    assert abs(tot) <= 4 * tsig, (tot, tsig)


def test_two_points_with_curved_rays_are_linear(ctx):
    """one point inside and one outside the shape: the connection of every path goes to the emitter K_event selected (the crossing
    Connector for the outside one), and the film is the sum of the two single-emitter films"""
    base = _curved(P.STEP_RK4, env_radiance=[0, 0, 0])
    _linear(ctx, base, P.point_emitter(PIN, I, 1.0), P.point_emitter(POUT, [2.0, 1.0, 0.5], 3.0))


def test_two_rectangles_are_linear(ctx):
    base = scenes.straight_scene(N=16, w=24, h=20, env_radiance=[0, 0, 0])
    _linear(ctx, base, P.area_emitter(RECT_ABOVE, [3.0, 2.0, 1.0], 1.0), P.area_emitter(RECT_BELOW, [1.0, 2.0, 4.0], 0.5))


def test_rectangle_hides_the_one_behind_it(ctx):
    """a small rectangle between the cube and a large one above: no light of the far one arrives through the near one.  The near one emits
    nothing and faces away, so a scene with both sees less than the far one alone, and exactly nothing of it in the near one's shadow
    column of a camera looking along it"""
    base = scenes.homogeneous_scene(w=24, h=20, env_radiance=[0, 0, 0])
    far = P.area_emitter(RECT_ABOVE, [3.0, 3.0, 3.0])
    near = P.area_emitter(np.array([[3.0, 0, 0, 0], [0, 0, 1, 1.5], [0, 3.0, 0, 0]], np.float64), [1e-3, 1e-3, 1e-3])    # faces up, covers the cube
    alone = _block_stats(_paths(ctx, base.copy(emitters=[far]), range(8), seed=5))[0]
    both = _block_stats(_paths(ctx, base.copy(emitters=[far, near]), range(8), seed=5))[0]
    assert alone.sum() > 0
    assert both.sum() < 1e-3 * alone.sum()


def test_transient_frames_sum_to_the_steady_film(ctx):
    ems = [P.area_emitter(RECT_ABOVE, [3.0, 2.0, 1.0]), P.area_emitter(RECT_BELOW, [1.0, 2.0, 4.0], 2.0), P.point_emitter(PIN, I), P.point_emitter([-0.5, -0.4, 0.3], I, 3.0)]
    p = scenes.homogeneous_scene(w=24, h=20, env_radiance=[0.2] * 3, decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=0.0, max_bound=64.0, bin_width=4.0, emitters=ems)
    sc, _ = ctx.upload_scene(p)
    film = ctx.render_to_host(sc, 0, 8, seed=5)
    ss, _ = ctx.upload_scene(p.copy(decomposition=P.DECOMPOSITION_NONE))
    steady = ctx.render_to_host(ss, 0, 8, seed=5)
    assert steady[..., :3].sum() > 0
    np.testing.assert_allclose(film[..., :-2].reshape(p.height, p.width, 16, 3).sum(2), steady[..., :3], rtol=1e-4, atol=1e-5)


def _multi_scene():
    ems = [P.area_emitter(RECT_ABOVE, [3.0, 2.0, 1.0]), P.area_emitter(RECT_BELOW, [1.0, 2.0, 4.0], 0.5), P.point_emitter(PIN, I), P.point_emitter([-0.5, -0.4, 0.3], I, 3.0)]
    return scenes.straight_scene(N=16, w=40, h=30, env_radiance=[0.2] * 3, emitters=ems)


def test_multi_context_uploads_the_list(ctx):
    p = _multi_scene()
    sc, vols = ctx.upload_scene(p)
    ref = ctx.render_to_host(sc, 0, 6, seed=2)
    m = capi.MultiContext([0, 0])
    try:
        msc, mv = m.upload_scene(p)
        film = m.render_to_host(msc, 0, 6, seed=2)
        assert ref[..., :3].sum() > 0
        assert np.allclose(film, ref, rtol=1e-4, atol=1e-5)                        # float summation order only
        for v in mv:
            v.destroy()
    finally:
        m.close()
    for v in vols:
        v.destroy()


def test_check_build_renders_the_list_in_bounds():
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for p in (_multi_scene(), _curved(P.STEP_RK4, emitters=[P.point_emitter(PIN, I), P.point_emitter(POUT, I, 3.0)])):
            sc, vols = c.upload_scene(p)
            f = c.render_to_host(sc, 0, 2, seed=1)
            assert np.isfinite(f).all()
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (kind, idx, lim)
            for v in vols:
                v.destroy()
    finally:
        c.close()


def test_library_refusals(ctx):
    """mer_render's own checks, past capi's validation: the exact outside test, the legacy fields beside the list, the cap"""
    p = scenes.homogeneous_scene(w=8, h=8, emitters=[P.area_emitter(RECT_ABOVE, [1, 1, 1])])
    sc, _ = ctx.upload_scene(p)
    ctx.render_to_host(sc, 0, 1)
    # a large rectangle cutting the cube off-centre: its corners and centre all lie outside
    sc._emitters_keep[0].to_world[:] = [3.0, 0, 0, 3.5, 0, 0, -1, 0.8, 0, 3.0, 0, 0]
    with pytest.raises(capi.MerError, match="must lie outside"):
        ctx.render_to_host(sc, 0, 1)
    # the same on a sphere (radius 1): the rectangle's corners and centre lie outside it, its closest point to the centre inside
    ps = scenes.homogeneous_scene(w=8, h=8, boundary=P.BOUNDARY_SPHERE, sph_radius=1.0, emitters=[P.area_emitter(RECT_ABOVE, [1, 1, 1])])
    sc, _ = ctx.upload_scene(ps)
    ctx.render_to_host(sc, 0, 1)
    sc._emitters_keep[0].to_world[:] = [3.0, 0, 0, 3.5, 0, 0, -1, 0.8, 0, 3.0, 0, 0]
    with pytest.raises(capi.MerError, match="must lie outside"):
        ctx.render_to_host(sc, 0, 1)
    sc._emitters_keep[0].to_world[:] = [3.0, 0, 0, 3.5, 0, 0, -1, 1.2, 0, 3.0, 0, 0]          # moved up to y = 1.2: clear of the sphere
    ctx.render_to_host(sc, 0, 1)
    sc, _ = ctx.upload_scene(p)
    sc.point_intensity[:] = [1, 1, 1]
    with pytest.raises(capi.MerError, match="must be zero"):
        ctx.render_to_host(sc, 0, 1)
    sc, _ = ctx.upload_scene(p)
    sc.n_emitters = 33
    with pytest.raises(capi.MerError, match="at most 32"):
        ctx.render_to_host(sc, 0, 1)
    sc, _ = ctx.upload_scene(p.copy(emitters=[P.point_emitter(PIN, I), P.point_emitter(PIN, I)]))
    sc._emitters_keep[1].sampling_weight = -1.0
    with pytest.raises(capi.MerError, match="samplingWeight"):
        ctx.render_to_host(sc, 0, 1)


# ---- the absolute value: GPU against tests/volpath64_multi.py, an independent float64 volpath of the same scene

RECT_NEAR = np.array([[0.6, 0, 0, 0.8], [0, 0, -1, 1.6], [0, -0.6, 0, 0]], np.float64)    # below RECT_ABOVE, facing down: hides part of it
MULTI_RECTS = [(RECT_ABOVE, 3.0, 1.0), (RECT_NEAR, 1.5, 0.5)]
# point emitters outside the cube (weights 1:3): inside a scattering medium a point emitter's I / r^2 has no finite variance, which no per-pixel
# z-test survives; rectangles and points outside the shape cannot share a scene, so they get one scene each
MULTI_POINTS = [([-1.6, 1.4, 0.4], 3.0, 1.0), ([1.5, -1.3, -0.6], 2.0, 3.0)]


@pytest.mark.parametrize("name", ["rectangles_env", "points_env"])
def test_render_matches_the_float64_volpath(ctx, name):
    """HG medium in the cube, the environment, no depth limit, and either two rectangles above the cube -- the nearer one hiding part of the
    farther one, weights 2:1 -- or two point emitters outside it (weights 1:3).  Per-pixel z-test of the means against tests/volpath64_multi.py
    -- which samples EVERY emitter at every vertex instead of selecting one -- with at most 1 + 1 % outliers beyond 4 sigma, and the image total"""
    from tests import volpath64_multi as vm
    cam = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
    pts, rcs = (MULTI_POINTS, []) if name == "points_env" else ([], MULTI_RECTS)
    p = scenes.homogeneous_scene(w=16, h=16, sigma_s=[1.0] * 3, sigma_a=[0.5] * 3, phase=P.PHASE_HG, g=0.5, env_radiance=[0.2] * 3, fov_x_deg=50.0,
                                 cam_to_world=cam, rfilter=P.FILTER_BOX, rfilter_param=0.5, max_depth=-1,
                                 emitters=[P.point_emitter(q, [i] * 3, w) for q, i, w in pts] + [P.area_emitter(m, [l] * 3, w) for m, l, w in rcs])
    S = 4096
    ref_m, ref_v = vm.render([(q, i) for q, i, _ in pts], [vm.Rect(m, l) for m, l, _ in rcs], 0.2, 1.0, 0.5, 0.5, 16, 16, 50.0, cam, spp=S, seed=1)
    sc, _ = ctx.upload_scene(p)
    K = 1024
    x = np.stack([ctx.render_paths(sc, k, seed=11)[..., 0] for k in range(K)]).astype(np.float64)
    z = (x.mean(0) - ref_m) / np.sqrt(x.var(0) / K + ref_v / S + 1e-14)
    assert (np.abs(z) > 4).sum() <= 1 + 0.01 * z.size, (np.abs(z).max(), (np.abs(z) > 4).sum())
    tg, tr = x.sum((1, 2)), ref_m.sum()
    assert abs(tg.mean() - tr) < 4 * np.sqrt(tg.var() / K + ref_v.sum() / S), (tg.mean(), tr)
    assert ref_m.mean() > 0.1
