"""Seeded random scene configurations (every switch of the scene description drawn independently) through mer_render_paths against the oracle: the
hand-written cases of tests/test_gpu_render.py cover each feature, this covers their COMBINATIONS (boundary x medium kind x phase x strategy x
estimator x stepper x RIF kind x emitters x depth rules x hideEmitters).  Same per-path thresholds as everywhere: >= 99 % of the paths within 1e-4
(>= 92 % when a curved-ray connection solver runs)."""
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, synth
from tests import scenes
from tests.test_oracle_kat import RECT_ABOVE

pytestmark = pytest.mark.gpu


def _random_scene(seed):
    r = np.random.RandomState(1000 + seed)
    pick = lambda *a: a[r.randint(len(a))]
    N = pick(12, 16, 24)
    kw = dict(width=pick(17, 24, 33), height=pick(13, 20, 24), rfilter=pick(P.FILTER_BOX, P.FILTER_GAUSSIAN), rfilter_param=0.5,
              max_depth=pick(-1, -1, 3, 4, 6), rr_depth=pick(5, 2, 50), hide_emitters=bool(pick(0, 0, 1)),
              phase=pick(P.PHASE_ISOTROPIC, P.PHASE_HG), g=float(pick(0.8, -0.4, 0.3)),
              env_radiance=pick([1.0, 1.0, 1.0], [0.0, 0.0, 0.0], [0.5, 0.7, 0.9]), fov_x_deg=float(pick(95.84, 40.0, 60.0)))
    sphere = pick(0, 0, 1)
    if sphere:
        kw.update(boundary=P.BOUNDARY_SPHERE, sph_radius=float(pick(0.8, 0.9)))
    curved = pick(0, 1, 1)
    grid_sigma = pick(0, 1, 1)
    if grid_sigma:
        kw.update(sigma_mode=P.SIGMA_GRID, density=synth.density_field(N), density_scale=float(pick(2.0, 4.0)), tr_estimator=pick(P.TR_RATIO, P.TR_WOODCOCK2),
                  albedo=pick([0.9, 0.9, 0.9], [0.95, 0.8, 0.6]))
        if pick(0, 0, 1):
            kw.update(albedo_mode=P.ALBEDO_GRID, albedo_grid=scenes.rgb_albedo(N, seed=seed))
        if pick(0, 0, 1):
            kw.update(emission=[0.2, 0.12, 0.06])
    else:
        kw.update(sigma_mode=P.SIGMA_HOMOGENEOUS, sigma_s=pick([0.5, 3.5, 7.5], [1.0, 1.0, 1.0]), sigma_a=pick([0.05] * 3, [0.0, 0.1, 0.3]),
                  strategy=pick(P.STRATEGY_BALANCE, P.STRATEGY_SINGLE, P.STRATEGY_MAXIMUM))
        if kw["strategy"] == P.STRATEGY_MAXIMUM and kw["sigma_s"] == [1.0, 1.0, 1.0] and kw["sigma_a"] == [0.05] * 3:
            kw["strategy"] = P.STRATEGY_BALANCE                     # MaxExpDist needs sigma_t to vary across the channels
    point = pick(0, 0, 1)
    if curved:
        kind = pick("trilinear", "trilinear", "bspline")
        if kind == "trilinear":
            kw.update(rif_mode=P.RIF_TRILINEAR, rif=pick(synth.linear_rif(N), synth.radial_rif(N)), stepper=pick(P.STEP_RK4, P.STEP_VERLET))
        else:
            kw.update(rif_mode=P.RIF_BSPLINE3, rif=synth.radial_rif(N, (-1.3,) * 3, (1.3,) * 3), rif_aabb=([-1.3] * 3, [1.3] * 3), stepper=pick(P.STEP_VERLET, P.STEP_RK4))
        kw.update(stepsize=0.5 * 2.0 / (N - 1))
        if pick(0, 0, 1):
            kw.update(boundary_bsdf=P.BSDF_HDIELECTRIC)
    else:
        if pick(0, 0, 1):
            kw.update(rif_const=1.33, boundary_bsdf=P.BSDF_HDIELECTRIC)
        elif pick(0, 1):
            kw.update(area_to_world=RECT_ABOVE, area_radiance=pick([3.0, 2.0, 1.0], [1.0, 1.0, 1.0]))
        if grid_sigma and pick(0, 0, 0, 1):
            kw.update(method=P.METHOD_SIMPSON)
    if point:
        inside = pick(1, 1, 0)
        kw.update(point_position=[0.2, 0.3, -0.1] if inside else [0.3, 1.6, -0.4], point_intensity=[1.0, 0.8, 0.5])
    layout = pick(capi.LAYOUT_DENSE, capi.LAYOUT_CELL8, capi.LAYOUT_BRICK27, capi.LAYOUT_AUTO)
    return P.SceneParams(**kw), layout, bool(curved and point)


@pytest.mark.parametrize("seed", range(40))
def test_random_scene_configuration_matches_oracle(ctx, orc, seed):
    p, layout, connections = _random_scene(seed)
    sc, vols = ctx.upload_scene(p, layout=layout)
    a = ctx.render_paths(sc, seed % 3, seed=seed)
    b = orc.render_paths(p, seed % 3, seed)
    assert np.isfinite(a).all()
    # method = simpson: the free flight is the root of a quadrature found by Newton / bisection to a tolerance; the GPU's and the oracle's roots differ in
    # the last bits (expf / logf ulps), a CONTINUOUS perturbation that a deep path (scale 4, no depth limit) carries to a few 1e-4 -- not a decision flip
    tol = 2e-3 if p.method == P.METHOD_SIMPSON else 1e-4
    close = np.abs(a - b).max(2) <= tol * np.maximum(1.0, np.abs(b).max(2))
    assert close.mean() > (0.90 if connections else 0.99), (seed, close.mean(), {k: v for k, v in p.__dict__.items() if not hasattr(v, "shape")})
    for v in vols:
        v.destroy()


@pytest.mark.parametrize("seed", range(24))
def test_random_scene_film_does_not_depend_on_the_scheduling(ctx, seed):
    """The same random configurations as FILMS, under the scheduling the render picks by itself (four pipelines, spawned side walks where they apply,
    fitted launch grids, batches of 4 passes) and under its opposite (one pipeline, every walk in the path's lane, full grids, batches of 8, a slot
    pool small enough to be refilled dozens of times; the march list spatially sorted when the rays are curved): the film is the same up to float summation
    order, every sample lands, and the work counters agree -- the scheduler moves work around, it never changes or loses any."""
    p, layout, connections = _random_scene(seed)
    sc, vols = ctx.upload_scene(p, layout=layout)
    spp = 6
    ctx.counters_reset(); fa = ctx.render_to_host(sc, 0, spp, seed=seed); ca = ctx.counters()
    with ctx.options(pipes=1, spawn_walks=0, grid_fit=0, check_every=8, nslots=2048, march_sort=2 if p.rif_mode != P.RIF_CONST else 0):
        ctx.counters_reset(); fb = ctx.render_to_host(sc, 0, spp, seed=seed); cb = ctx.counters()
    assert np.isfinite(fa).all() and np.isfinite(fb).all()
    scale = max(float(np.abs(fb[..., :3]).max()), 1e-6)
    assert np.abs(fa[..., :3] - fb[..., :3]).max() <= 5e-4 * scale, (seed, float(np.abs(fa[..., :3] - fb[..., :3]).max()), scale)
    assert np.allclose(fa[..., 3:], fb[..., 3:], rtol=1e-4, atol=1e-5)                      # alpha and weight
    for k in (capi.C_PATHS, capi.C_REAL):
        assert ca[k] == cb[k], (seed, k, ca[k], cb[k])
    # a side walk whose prefactor is zero (a look-up that the depth limit blocks) is not spawned at all, where the in-lane form walks and then discards
    # the result: the spawning render does at most the other one's marching work (equal when nothing is blocked)
    for k in (capi.C_TENTATIVE, capi.C_STEPS):
        assert ca[k] <= cb[k], (seed, k, ca[k], cb[k])
        if p.max_depth < 0:
            assert ca[k] == cb[k], (seed, k, ca[k], cb[k])
    for v in vols:
        v.destroy()


# ---- the EXTRA kernels (emitter lists, spots, envmap, rough boundary, signed-distance boundary, the sensors beside the pinhole, modulation): the
#      oracle knows none of them, so the random scenes of tests/fuzz_scenes.py are held to what the code promises of itself -- include/mer.h: no
#      context option changes a per-path result; shards add up; a film is the filtered sum of its paths; a context carries nothing from one scene
#      into the next; no index leaves its buffer
from tests import fuzz_scenes as F       # noqa: E402

BIG = [(33, 40), (48, 40)]               # 2 and 4 tiles of 32 x 32: 2048 and 4096 work ids against a pool of 1024 slots


def _destroy(vols):
    for v in vols:
        v.destroy()


def _differ(a, b):
    bad = np.argwhere((a != b).any(-1))
    return "%d of %d paths differ, first (y, x) %s: %s vs %s" % (len(bad), a.shape[0] * a.shape[1], bad[0], a[tuple(bad[0])], b[tuple(bad[0])])


@pytest.mark.parametrize("seed", range(48))
def test_extra_scene_paths_do_not_depend_on_the_scheduling(ctx, seed):
    """per-path radiance of a random EXTRA scene, bit for bit, under every context option that reaches it: one pipeline on a pool of 1024 slots
    with full grids and batches of 8 (refilled on the two larger images: K_event's regeneration draws what K_gen draws), short passes, the
    longer tail, K_gen handing every sample on, two-kernel walks, one and five K_connect launches per pass, global loads, the dense layout"""
    p, layout, tags = F.random_extra_scene(seed)
    sc, vols = ctx.upload_scene(p, layout=layout)
    s = seed % 3
    a = ctx.render_paths(sc, s, seed=seed)
    assert np.isfinite(a).all() and a.max() > 0, (seed, sorted(tags))

    def same(scene=sc, **opts):
        with ctx.options(**opts):
            b = ctx.render_paths(scene, s, seed=seed)
        assert np.array_equal(a, b), (seed, opts, sorted(tags), _differ(a, b))

    with ctx.options(pipes=1, nslots=1024, grid_fit=0, check_every=8):
        ctx.counters_reset(); b = ctx.render_paths(sc, s, seed=seed); c = ctx.counters()
    assert np.array_equal(a, b), (seed, "small pool", sorted(tags), _differ(a, b))
    if (p.width, p.height) in BIG:
        assert c[capi.C_PATHS] > 1024, (seed, c[capi.C_PATHS])                 # the pool was refilled
    same(ksteps=16)
    same(adaptive_k=1)
    same(gen_all=1)
    if p.rif_mode == P.RIF_CONST and p.sigma_mode == P.SIGMA_GRID:
        same(inline_walks=0)
    if F.connect_stage(p):
        same(connect_launches=1)
        same(connect_launches=5)
    if p.rif_mode == P.RIF_TRILINEAR:
        with ctx.options(buffer_loads=0):
            s2, v2 = ctx.upload_scene(p, layout=layout)
            b = ctx.render_paths(s2, s, seed=seed)
        assert np.array_equal(a, b), (seed, "buffer_loads=0", sorted(tags), _differ(a, b))
        s3, v3 = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
        b = ctx.render_paths(s3, s, seed=seed)
        assert np.array_equal(a, b), (seed, "dense layout", sorted(tags), _differ(a, b))
        _destroy(v2 + v3)
    _destroy(vols)


@pytest.mark.parametrize("curved", [0, 1])
def test_gen_all_renders_no_work_id_outside_the_image(ctx, curved):
    """K_gen and its gen_all switch are one template for every kernel set: on the kernels of a plain scene (pinhole, constant environment, no
    emitter list) a 33 x 20 image fills two 32 x 32 tiles partly, in x and in y, and 2048 - 660 work ids fall outside it.  gen_all = 1 must
    hand none of them to K_event, which replays an id without asking whether its pixel exists: the paths are bit for bit those of gen_all = 0,
    and the film (Gaussian splats, 3 samples) the same up to summation order, weight included."""
    N = 12
    kw = dict(width=33, height=20, density=synth.density_field(N), rfilter=P.FILTER_GAUSSIAN, rfilter_param=0.5)
    if curved:
        kw.update(rif_mode=P.RIF_TRILINEAR, rif=synth.linear_rif(N), stepsize=0.5 * 2.0 / (N - 1))
    p = P.SceneParams(**kw)
    sc, vols = ctx.upload_scene(p)
    a = ctx.render_paths(sc, 1, seed=5)
    fa = ctx.render_to_host(sc, 0, 3, seed=5)
    with ctx.options(gen_all=1):
        b = ctx.render_paths(sc, 1, seed=5)
        fb = ctx.render_to_host(sc, 0, 3, seed=5)
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(a, b), _differ(a, b)
    _films_agree(fb, fa, "gen_all=1")
    _destroy(vols)


def _films_agree(fa, fb, what):
    """the film tolerance of the scheduling tests: RGB of every frame within 5e-4 of the largest value, alpha and weight to 1e-4 / 1e-5"""
    assert np.isfinite(fa).all() and np.isfinite(fb).all(), what
    scale = max(float(np.abs(fb[..., :-2]).max()), 1e-6)
    err = float(np.abs(fa[..., :-2] - fb[..., :-2]).max())
    assert err <= 5e-4 * scale, (what, err, scale)
    assert np.allclose(fa[..., -2:], fb[..., -2:], rtol=1e-4, atol=1e-5), what


@pytest.mark.parametrize("seed", range(24))
def test_extra_scene_film_does_not_depend_on_the_scheduling(ctx, seed):
    """the film of a random EXTRA scene under the scheduling the render picks by itself and under its opposite (one pipeline, full grids, batches
    of 8, a pool of 2048 slots): the same up to float summation order, every sample lands, the work counters agree.  And it is the sum of its
    shards -- two sample-interleaved ones, three tile ones (a Gaussian splat crosses the tile borders of the two larger images)."""
    p, layout, tags = F.random_extra_scene(seed)
    sc, vols = ctx.upload_scene(p, layout=layout)
    spp = 6
    ctx.counters_reset(); fa = ctx.render_to_host(sc, 0, spp, seed=seed); ca = ctx.counters()
    with ctx.options(pipes=1, grid_fit=0, check_every=8, nslots=2048):
        ctx.counters_reset(); fb = ctx.render_to_host(sc, 0, spp, seed=seed); cb = ctx.counters()
    assert fa.shape[2] == 3 * F.film_frames(p) + 2
    assert fa[..., :-2].max() > 0, (seed, sorted(tags))
    _films_agree(fa, fb, (seed, sorted(tags)))
    for k in (capi.C_PATHS, capi.C_REAL):
        assert ca[k] == cb[k], (seed, k, ca[k], cb[k])
    parts = sum(ctx.render_to_host(sc, r, 3, seed=seed, spp_stride=2) for r in range(2))
    assert np.allclose(fa, parts, rtol=1e-4, atol=1e-5), (seed, "sample shards", float(np.abs(fa - parts).max()))
    tiles = sum(ctx.render_to_host(sc, 0, spp, seed=seed, tile_rank=r, tile_count=3) for r in range(3))
    assert np.allclose(fa, tiles, rtol=1e-4, atol=1e-5), (seed, "tile shards", float(np.abs(fa - tiles).max()))
    _destroy(vols)


ONE_FRAME_BOX = F.one_frame_box_seeds(range(24))


@pytest.mark.parametrize("seed", ONE_FRAME_BOX)
def test_extra_scene_film_is_the_sum_of_its_paths(ctx, seed):
    """the two output routes of the EXTRA kernels: path_out (mer_render_paths) and the splats of K_gen, K_event and K_connect.  Under the box
    filter of radius 0.5 a splat stays in its pixel with one constant table weight w0, and the film's sample s is the path of
    mer_render_paths(s) (the same (seed, pixel, sample) stream): film RGB / weight = the mean of the four paths, up to float32 re-summation.
    The box's radius is 0.5 + 1e-5 (filter_table): a sample within 1e-5 of a pixel edge also lands in the neighbour beyond it -- 4e-5 of the
    samples, 0.3 pixels per scene here (seed 17 has one).  Such a pixel shows in its weight, (4 + 1) w0; it is held to the same tolerance
    with the one neighbouring path that accounts for its surplus, and there may be at most 3 of them."""
    assert len(ONE_FRAME_BOX) >= 6
    p, layout, tags = F.random_extra_scene(seed)
    sc, vols = ctx.upload_scene(p, layout=layout)
    film = ctx.render_to_host(sc, 0, 4, seed=seed)
    paths = np.stack([ctx.render_paths(sc, s, seed=seed) for s in range(4)])
    assert film.shape[2] == 5 and paths.max() > 0
    w0 = float(np.median(film[..., 4])) / 4
    assert abs(w0 - 1) < 1e-3
    own = np.isclose(film[..., 4], 4 * w0, rtol=1e-5)
    crossed = np.argwhere(~own)
    print("   seed %d: %d pixels with a neighbour's sample" % (seed, len(crossed)))
    assert len(crossed) <= 3, (seed, len(crossed))
    np.testing.assert_allclose((film[..., :3] / film[..., 4:5])[own], paths.mean(0)[own], rtol=1e-4, atol=1e-5, err_msg=str((seed, sorted(tags))))
    for y, x in crossed:
        assert np.isclose(film[y, x, 4], 5 * w0, rtol=1e-5), (seed, y, x, film[y, x, 4])
        near = [paths[s, y + dy, x + dx] for s in range(4) for dy, dx in ((0, 1), (0, -1), (1, 0), (-1, 0)) if 0 <= y + dy < p.height and 0 <= x + dx < p.width]
        want = (paths[:, y, x].sum(0)[None] + np.stack(near)) / 5
        assert np.isclose(film[y, x, :3] / film[y, x, 4], want, rtol=1e-4, atol=1e-5).all(1).any(), (seed, y, x)
    _destroy(vols)


def test_context_state_does_not_leak_between_scenes(ctx):
    """what a context keeps from render to render -- the emitter table and the filter table it re-uploads on a mismatch, envmaps behind handles,
    the slot pool and the work lists -- must not reach the next scene: six scenes that differ pairwise in all of it, rendered in order, in
    reverse order, and again after the second one's volumes and map were destroyed and uploaded anew, give the same arrays every time"""
    ps = [F.random_extra_scene(s) for s in F.LEAK_SEEDS]
    up = [ctx.upload_scene(p, layout=layout) for p, layout, _ in ps]
    paths = lambda i: ctx.render_paths(up[i][0], 1, seed=F.LEAK_SEEDS[i])
    film = lambda i: ctx.render_to_host(up[i][0], 0, 4, seed=F.LEAK_SEEDS[i])
    first = [paths(i) for i in range(6)]
    assert all(np.isfinite(a).all() and a.max() > 0 for a in first)
    for i in reversed(range(6)):
        assert np.array_equal(paths(i), first[i]), (F.LEAK_SEEDS[i], "reverse order")
    ffirst = [film(i) for i in range(6)]
    for i in reversed(range(6)):
        _films_agree(film(i), ffirst[i], (F.LEAK_SEEDS[i], "films, reverse order"))
    _destroy(up[1][1])
    up[1] = ctx.upload_scene(ps[1][0], layout=ps[1][1])
    assert np.array_equal(paths(1), first[1]) and np.array_equal(paths(0), first[0]), "after the re-upload"
    _films_agree(film(1), ffirst[1], "film of the re-uploaded scene")
    _films_agree(film(0), ffirst[0], "film after the re-upload")
    for _, vols in up:
        _destroy(vols)


@pytest.fixture(scope="module")
def cctx():
    c = capi.Context(0, check=True)
    en, *_ = c.debug_bounds()
    assert en, "libmer_check.so was built without -DMER_BOUNDS_CHECK"
    yield c
    c.close()


@pytest.mark.parametrize("seed", F.BOUNDS_SEEDS)
def test_extra_scenes_stay_in_bounds(cctx, ctx, seed):
    """the bounds-checking build on random EXTRA scenes: per-path radiance bit for bit that of the product build, a film of 5 samples (four
    pipelines), and no index outside its buffer in either"""
    p, layout, tags = F.random_extra_scene(seed)
    sc, vols = cctx.upload_scene(p, layout=layout)
    s2, v2 = ctx.upload_scene(p, layout=layout)
    a = cctx.render_paths(sc, 0, seed=seed)
    en, n, kind, idx, lim = cctx.debug_bounds()
    assert n == 0, (seed, sorted(tags), "paths", kind, idx, lim)
    b = ctx.render_paths(s2, 0, seed=seed)
    assert np.array_equal(a, b), (seed, sorted(tags), _differ(a, b))
    f = cctx.render_to_host(sc, 0, 5, seed=seed)
    en, n, kind, idx, lim = cctx.debug_bounds()
    assert n == 0, (seed, sorted(tags), "film", kind, idx, lim)
    assert np.isfinite(f).all() and f[..., :-2].max() > 0
    _destroy(vols + v2)
