"""The rough dielectric boundary (hroughdielectric) on the HIP path, through the C-ABI: the leaf BSDF against the float64 restatement
tests/microfacet64.py (values, sampler consistency, the reference's chi^2 fixture, albedo), and renders -- the smooth limit against
hdielectric, curved rays in a constant index against straight rays, scheduling options, bounds, and the XML path."""
import os
import numpy as np
import pytest
from mitsubaer_amd import capi, host, params as P, synth
from tests import microfacet64 as mf, scenes

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KINDS = [(P.MICROFACET_BECKMANN, True), (P.MICROFACET_BECKMANN, False), (P.MICROFACET_GGX, True), (P.MICROFACET_GGX, False),
         (P.MICROFACET_PHONG, False)]


def _desc(kind, alpha, visible):
    s = capi.SceneDesc()
    s.rough_distribution = kind; s.rough_alpha = alpha; s.rough_sample_visible = int(visible)
    return s


def _dirs(n, seed, upper=None):
    v = np.random.RandomState(seed).normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if upper is not None:
        v[:, 2] = np.abs(v[:, 2]) * (1 if upper else -1)
    return v.astype(np.float32)


def _away_from_edges(eta, wi, wo, eps=1e-2):
    """away from grazing: |cos| > 1e-2 for wi, wo and for both against the half vector and its own inclination (at those edges a float32
    rounding flips which side a vector is on and a value between 0 and non-zero), and cos^2 theta_t > 1e-2 at the microfacet (near total
    internal reflection 1 - F cancels in float32 as it does in the reference's float32 code)"""
    eta = np.float32(eta)
    H = mf.half_vector(eta, wi, wo)
    wiH = np.sum(wi * H, 1)
    cosT2 = 1 - (1 - wiH * wiH) * np.where(wiH > 0, 1 / np.float64(eta), np.float64(eta)) ** 2
    c = [np.abs(wi[:, 2]), np.abs(wo[:, 2]), np.abs(wiH), np.abs(np.sum(wo * H, 1)), np.abs(H[:, 2]), np.abs(cosT2)]
    return np.all([x > eps for x in c], 0)


@pytest.mark.parametrize("kind,visible", KINDS)
@pytest.mark.parametrize("eta", [1.33, 1.5, 2.4])
def test_leaf_eval_and_pdf_against_float64(ctx, kind, visible, eta):
    """both hemispheres for wi (interior hits see 1 / eta) and wo; rtol 2e-4 away from grazing (|cos| > 1e-2)"""
    n = 60000
    for alpha in (0.1, 0.3, 0.7):
        wi = _dirs(n, 1); wo = _dirs(n, 2)
        val, pdf = ctx.rough_eval(_desc(kind, alpha, visible), eta, wi, wo)
        d = mf.Distr(kind, alpha, visible)
        rv, rp = mf.eval_pdf(d, np.float32(eta), wi.astype(np.float64), wo.astype(np.float64))
        keep = _away_from_edges(eta, wi, wo)
        assert np.isfinite(val).all() and np.isfinite(pdf).all() and (val >= 0).all() and (pdf >= 0).all()
        # conditioning: in the far tail of a narrow lobe (D ~ exp(-tan^2 / alpha^2)) a float32 rounding of the half vector alone moves the
        # value by more than 2e-4; the float64 values at inputs moved by a few float32 ulps bound that part
        rs = np.random.RandomState(7)
        sens_v = np.zeros(n); sens_p = np.zeros(n)
        for _ in range(4):
            jit = lambda v: (lambda x: x / np.linalg.norm(x, axis=1, keepdims=True))(v.astype(np.float64) + 2.4e-7 * rs.normal(size=v.shape))
            v2, p2 = mf.eval_pdf(d, np.float32(eta), jit(wi), jit(wo))
            sens_v = np.maximum(sens_v, np.abs(v2 - rv)); sens_p = np.maximum(sens_p, np.abs(p2 - rp))
        for g, r, sens in ((val, rv, sens_v), (pdf, rp, sens_p)):
            # below 1e-20 float32 loses the value to underflow (Beckmann / Phong tails: exp(-tan^2 / alpha^2)): an absolute bound there
            err = np.abs(g - r)[keep]; tol = 2e-4 * np.abs(r[keep]) + 4 * sens[keep] + 1e-20
            assert np.all(err <= tol), (alpha, np.sum(err > tol), np.max(err / np.maximum(np.abs(r[keep]), 1e-20)))
            big = r[keep] > 1e-20
            assert np.median(err[big] / r[keep][big]) < 2e-5
        assert (rv[keep] > 0).sum() > n / 4


@pytest.mark.parametrize("kind,visible", KINDS)
@pytest.mark.parametrize("eta", [1.33, 2.4])
def test_leaf_sample_is_consistent_with_eval_and_pdf(ctx, kind, visible, eta):
    n = 100000
    for alpha in (0.1, 0.4):
        wi = _dirs(n, 3); u3 = np.random.RandomState(4).rand(n, 3).astype(np.float32)
        wo, w, pdf = ctx.rough_sample(_desc(kind, alpha, visible), eta, wi, u3)
        assert np.isfinite(wo).all() and np.isfinite(w).all() and np.isfinite(pdf).all() and (w >= 0).all()
        ok = (w > 0) & _away_from_edges(eta, wi, wo)
        assert ok.mean() > 0.6
        assert np.allclose(np.linalg.norm(wo[w > 0], axis=1), 1, atol=1e-5)
        rv, rp = mf.eval_pdf(mf.Distr(kind, alpha, visible), np.float32(eta), wi[ok].astype(np.float64), wo[ok].astype(np.float64))
        for g, r in ((pdf[ok], rp), (w[ok], rv / rp)):
            bad = np.abs(g - r) > 1e-3 * np.abs(r)
            assert not bad.any(), (alpha, bad.sum(), np.max(np.abs(g - r) / np.abs(r)))
        # the same numbers in float64 pick the same branch (reflection / refraction / no sample) nearly always
        rwo, rw, _, _ = mf.sample(mf.Distr(kind, alpha, visible), np.float32(eta), wi.astype(np.float64), u3.astype(np.float64))
        assert ((rw > 0) == (w > 0)).mean() > 0.999 and (np.sign(rwo[:, 2]) == np.sign(wo[:, 2]))[w > 0].mean() > 0.999


def test_total_internal_reflection_has_no_refraction_branch(ctx):
    """from inside beyond the critical angle of a nearly smooth surface: every sample reflects (the refraction branch weighs 0)"""
    n = 20000
    s = np.sin(np.radians(60.0))
    wi = np.tile(np.array([[s, 0.0, -np.sqrt(1 - s * s)]], np.float32), (n, 1))         # 60 degrees, critical angle of 1.5: 41.8
    for kind, visible in KINDS:
        wo, w, pdf = ctx.rough_sample(_desc(kind, 1e-3, visible), 1.5, wi, np.random.RandomState(5).rand(n, 3).astype(np.float32))
        assert (w > 0).mean() > 0.99
        assert (wo[w > 0, 2] < 0).all()
        assert abs(w.mean() - 1.0) < 2e-2, (kind, visible, w.mean())       # all energy reflected


@pytest.mark.parametrize("kind,visible", KINDS)
@pytest.mark.parametrize("upper", [True, False])
def test_chisquare_reference_fixture(ctx, kind, visible, upper):
    """data/tests/test_bsdf.xml:80-101 of the reference: roughdielectric with beckmann, phong and ggx at alpha = 0.3, intIOR 1.5 (a constant RIF
    of 1.5), both samplers, wi in both hemispheres; the protocol of src/tests/test_chisquare.cpp (10 x 20 cells, pooling below 5 expected
    samples), significance level 1 - (1 - 0.0025)^(1/20) per incident direction as the reference uses"""
    d = mf.Distr(kind, 0.3, visible)
    rng = np.random.RandomState(21)
    n = 200000
    for wi in _dirs(3, 30 + upper, upper):
        wo, w, _ = ctx.rough_sample(_desc(kind, 0.3, visible), 1.5, np.repeat(wi[None], n, 0), rng.rand(n, 3).astype(np.float32))
        pval, level = mf.chi2_sphere(wo, w > 0, n, mf.chi2_pdf(d, 1.5, wi.astype(np.float64)))
        assert pval >= level, (pval, level, wi)


@pytest.mark.parametrize("kind,visible", KINDS)
def test_directional_albedo(ctx, kind, visible):
    """mean sample weight = the float64 quadrature of eval over the sphere, within 4 sigma"""
    n = 400000
    for wi, eta in ((np.array([0.2, 0.4, 0.89]), 1.5), (np.array([0.5, -0.3, -0.81]), 1.5), (np.array([0.1, 0.7, 0.3]), 2.4)):
        wi = (wi / np.linalg.norm(wi)).astype(np.float32)
        _, w, _ = ctx.rough_sample(_desc(kind, 0.3, visible), eta, np.repeat(wi[None], n, 0), np.random.RandomState(6).rand(n, 3).astype(np.float32))
        a = mf.albedo(mf.Distr(kind, 0.3, visible), np.float32(eta), wi.astype(np.float64))
        assert abs(w.mean() - a) < 4 * w.std() / np.sqrt(n) + 2e-3 * a, (w.mean(), a)


def test_leaf_refuses_bad_parameters(ctx):
    with pytest.raises(capi.MerError, match="distribution"):
        ctx.rough_eval(_desc(3, 0.3, 0), 1.5, _dirs(4, 1), _dirs(4, 2))
    with pytest.raises(capi.MerError, match="alpha"):
        ctx.rough_sample(_desc(0, -1.0, 0), 1.5, _dirs(4, 1), np.zeros((4, 3), np.float32))


# ---- renders

BOX = ([-1.05] * 3, [1.05] * 3)


def _sdf(N=48, radius=0.9):
    return -synth.sphere_sdf(N, radius=radius, aabb_min=BOX[0], aabb_max=BOX[1])


def _rough(p, kind=P.MICROFACET_GGX, alpha=0.2, visible=True):
    p.boundary_bsdf = P.BSDF_HROUGHDIELECTRIC
    p.rough_distribution = kind; p.rough_alpha = alpha; p.rough_sample_visible = visible
    return p


def _paths(ctx, p, K, seed):
    sc, vols = ctx.upload_scene(p)
    out = np.stack([ctx.render_paths(sc, k, seed=seed)[..., :3].sum(-1) for k in range(K)])
    for v in vols:
        v.destroy()
    return out


def _blocks_agree(a, b, blk=4, z=4.0):
    """per 4x4 block mean of the per-path radiance: z-test of two independent estimates; few outliers, and the image totals agree"""
    K, H, W = a.shape
    def stat(x):
        x = x[:, :H // blk * blk, :W // blk * blk].reshape(K, H // blk, blk, W // blk, blk).transpose(1, 3, 0, 2, 4).reshape(H // blk, W // blk, -1)
        return x.mean(-1), x.var(-1) / x.shape[-1]
    ma, va = stat(a); mb, vb = stat(b)
    zz = np.abs(ma - mb) / np.sqrt(va + vb + 1e-12)
    assert (zz > z).sum() <= 1 + 0.01 * zz.size, (zz.max(), (zz > z).sum(), zz.size)
    ta, tb = a.sum((1, 2)), b.sum((1, 2))
    assert abs(ta.mean() - tb.mean()) < z * np.sqrt(ta.var() / K + tb.var() / K) + 1e-9, (ta.mean(), tb.mean())


LIMIT = {
    "straight_homogeneous": lambda: scenes.homogeneous_scene(w=32, h=24, rif_const=1.5, sigma_s=[1.0, 1.5, 2.0], sigma_a=[0.1] * 3),
    "straight_grid": lambda: scenes.straight_scene(N=16, w=32, h=24, rif_const=1.33),
    "curved_trilinear": lambda: scenes.curved_scene(N=16, w=32, h=24, rif="radial"),
    "curved_bspline": lambda: scenes.bspline_scene(N=16, w=32, h=24),
    "curved_acoustic": lambda: scenes.homogeneous_scene(w=32, h=24, rif_mode=P.RIF_ACOUSTIC, ac_n_o=1.33, ac_n_max=0.02, ac_k_r=3.0, ac_mode=1,
                                                        stepsize=0.02, sigma_s=[1.0, 1.0, 1.0], sigma_a=[0.1] * 3),
    "sdf": lambda: scenes.straight_scene(N=16, w=32, h=24, rif_const=1.33, boundary=P.BOUNDARY_SDF, sdf=_sdf(), sdf_aabb=BOX),
}


@pytest.mark.parametrize("name", sorted(LIMIT))
def test_smooth_limit_equals_hdielectric(ctx, name):
    """alpha -> 1e-4: the rough boundary renders what the smooth one does (no point emitter: same estimator), per 4x4 block"""
    a = LIMIT[name](); a.boundary_bsdf = P.BSDF_HDIELECTRIC
    b = _rough(LIMIT[name](), P.MICROFACET_BECKMANN if name.startswith("curved") else P.MICROFACET_GGX, alpha=1e-4)
    K = 48
    _blocks_agree(_paths(ctx, a, K, seed=1), _paths(ctx, b, K, seed=2))


def _point(p):
    p.point_position = [-1.6, 1.4, 0.4]; p.point_intensity = [3.0, 2.5, 2.0]; p.env_radiance = [0.2, 0.2, 0.2]
    return p


def test_curved_in_a_constant_index_equals_straight(ctx):
    """a rough boundary with the outside point emitter: curved rays through a constant-index grid render what straight rays with that rif_const do"""
    N = 8
    kw = dict(w=32, h=24, sigma_s=[1.0, 1.5, 2.0], sigma_a=[0.1] * 3, phase=P.PHASE_HG, g=0.5)
    a = _rough(_point(scenes.homogeneous_scene(rif_const=1.4, **kw)))
    b = _rough(_point(scenes.homogeneous_scene(rif_mode=P.RIF_TRILINEAR, rif=np.full((N, N, N), 1.4, np.float32), stepsize=0.05, **kw)))
    K = 48
    _blocks_agree(_paths(ctx, a, K, seed=3), _paths(ctx, b, K, seed=4))


def test_outside_point_emitter_lights_the_straight_scene_through_the_rough_boundary(ctx):
    """the new transport: with a black environment all light comes from the point emitter through the surface vertex"""
    p = _rough(_point(scenes.homogeneous_scene(w=32, h=24, rif_const=1.5, sigma_s=[1.0] * 3, sigma_a=[0.1] * 3)))
    p.env_radiance = [0.0, 0.0, 0.0]
    x = _paths(ctx, p, 16, seed=5)
    assert np.isfinite(x).all() and x.mean() > 0


ROUGH_SCENES = {
    "straight": lambda: _rough(_point(scenes.straight_scene(N=16, w=40, h=32, rif_const=1.33))),
    "curved": lambda: _rough(_point(scenes.curved_scene(N=16, w=40, h=32, rif="radial")), P.MICROFACET_BECKMANN, 0.3, False),
}


@pytest.mark.parametrize("name", sorted(ROUGH_SCENES))
def test_scheduling_options_change_no_per_path_result(name):
    p = ROUGH_SCENES[name]()
    ref = None
    for opts in ({}, dict(pipes=1), dict(nslots=4096), dict(ksteps=16), dict(check_every=1), dict(inline_walks=0), dict(grid_fit=0)):
        c = capi.Context(0, **opts)
        sc, vols = c.upload_scene(p)
        out = np.stack([c.render_paths(sc, k, seed=9) for k in range(3)])
        for v in vols:
            v.destroy()
        c.close()
        assert np.isfinite(out).all()
        if ref is None:
            ref = out; assert ref.max() > 0
        else:
            assert np.array_equal(out, ref), opts


def test_bounds_check_renders_rough_scenes_clean():
    c = capi.Context(0, check=True)
    en, *_ = c.debug_bounds()
    assert en
    for p in (_rough(_point(scenes.homogeneous_scene(w=32, h=24, rif_const=1.5))),
              _rough(_point(scenes.curved_scene(N=16, w=32, h=24, rif="radial", boundary=P.BOUNDARY_SPHERE, sph_radius=0.95))),
              _rough(_point(scenes.straight_scene(N=16, w=32, h=24, rif_const=1.33, boundary=P.BOUNDARY_SDF, sdf=_sdf(), sdf_aabb=BOX)))):
        p.decomposition = P.DECOMPOSITION_TRANSIENT; p.min_bound = 0.0; p.max_bound = 12.0; p.bin_width = 0.5
        sc, vols = c.upload_scene(p)
        f = c.render_to_host(sc, 0, 8, seed=1)
        assert np.isfinite(f).all() and f[..., :-2].sum() > 0
        en, nviol, kind, idx, lim = c.debug_bounds()
        assert nviol == 0, (kind, idx, lim)
        for v in vols:
            v.destroy()
    c.close()


def test_point_emitter_inside_is_refused_by_the_render(ctx):
    p = _rough(scenes.homogeneous_scene(w=8, h=8, rif_const=1.5))
    sc, _ = ctx.upload_scene(p)
    sc.point_position[:] = [0.1, 0.2, 0.0]; sc.point_intensity[:] = [1.0, 1.0, 1.0]      # past capi's own check: mer_render refuses it
    with pytest.raises(capi.MerError, match="outside"):
        ctx.render_to_host(sc, 0, 1)
    sc.point_position[:] = [0.1, 3.0, 0.0]
    assert np.isfinite(ctx.render_to_host(sc, 0, 1)).all()
    # the signed-distance shape: mer_render looks the grid up at the emitter
    p = _rough(scenes.homogeneous_scene(w=8, h=8, rif_const=1.5, boundary=P.BOUNDARY_SDF, sdf=_sdf(), sdf_aabb=BOX))
    sc, _ = ctx.upload_scene(p)
    sc.point_position[:] = [0.1, 0.2, 0.0]; sc.point_intensity[:] = [1.0, 1.0, 1.0]
    with pytest.raises(capi.MerError, match="outside"):
        ctx.render_to_host(sc, 0, 1)
    sc.point_position[:] = [0.0, 0.97, 0.0]                    # inside the grid's box, outside the shape (radius 0.9)
    assert np.isfinite(ctx.render_to_host(sc, 0, 1)).all()


def test_xml_scene_through_the_product(ctx):
    """scenes/cfg_rough_boundary.xml through libmer_host equals the same scene built through params"""
    xml = os.path.join(ROOT, "scenes", "cfg_rough_boundary.xml")
    d, _ = host.flatten_xml(xml, {"samples": 4})
    film = host.render_xml(xml, {"samples": 4}, seed=7)
    assert np.isfinite(film).all() and film[..., :-2].sum() > 0
    p = scenes.homogeneous_scene(w=96, h=96, boundary=P.BOUNDARY_SPHERE, rif_mode=P.RIF_ACOUSTIC, ac_n_o=1.33, ac_n_max=0.02,
                                 ac_k_r=float(d.ac_k_r), ac_mode=1, stepsize=0.02, sigma_s=[1.5, 2.0, 2.5], sigma_a=[0.05] * 3,
                                 phase=P.PHASE_HG, g=0.6, env_radiance=[0.1] * 3, point_position=[-1.5, 2.0, 0.5], point_intensity=[8.0, 7.0, 6.0],
                                 fov_x_deg=60.0, cam_to_world=P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0]), rfilter=P.FILTER_BOX, rfilter_param=0.5,
                                 decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=2.0, max_bound=12.0, bin_width=0.25, max_depth=-1,
                                 stepper=P.STEP_VERLET, tr_estimator=P.TR_WOODCOCK2)           # the XML defaults
    _rough(p, P.MICROFACET_GGX, 0.2, True)
    sc, vols = ctx.upload_scene(p)
    ref = ctx.render_to_host(sc, 0, 4, seed=7)
    assert np.allclose(film, ref, rtol=1e-4, atol=1e-5)


# ---- the emitter sample at the surface vertex against independent float64 references

def _cube_scene(kind, alpha, visible, **kw):
    base = dict(w=16, h=16, sigma_s=[1.0] * 3, sigma_a=[0.1] * 3, phase=P.PHASE_ISOTROPIC, rif_const=1.5, env_radiance=[0.2] * 3,
                point_position=[-1.6, 1.4, 0.4], point_intensity=[3.0] * 3, fov_x_deg=50.0, cam_to_world=P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0]),
                rfilter=P.FILTER_BOX, rfilter_param=0.5, max_depth=6, rr_depth=100)
    base.update(kw)
    return _rough(scenes.homogeneous_scene(**base), kind, alpha, visible)


@pytest.mark.parametrize("kind,alpha,visible", [(P.MICROFACET_GGX, 0.3, True), (P.MICROFACET_BECKMANN, 0.2, False)])
def test_render_matches_the_float64_volpath(ctx, kind, alpha, visible):
    """tests/volpath64_rough.py (16 x 16 px, 4096 paths per pixel, max_depth 6): per-pixel z-test of the means with at most 1 + 1 % outliers
    beyond 4 sigma, and the image total; then the transient decomposition of the same scene, per-frame image totals within 4 sigma"""
    from tests import volpath64_rough as vp
    p = _cube_scene(kind, alpha, visible)
    ref_m, ref_v = vp.render(mf.Distr(kind, alpha, visible), spp=4096, seed=1, cam_to_world=p.cam_to_world)
    sc, _ = ctx.upload_scene(p)
    K = 512
    x = np.stack([ctx.render_paths(sc, k, seed=11)[..., 0] for k in range(K)])
    z = (x.mean(0) - ref_m) / np.sqrt(x.var(0) / K + ref_v / 4096 + 1e-14)
    assert (np.abs(z) > 4).sum() <= 1 + 0.01 * z.size, (np.abs(z).max(), (np.abs(z) > 4).sum())
    tg, tr = x.sum((1, 2)), ref_m.sum()
    assert abs(tg.mean() - tr) < 4 * np.sqrt(tg.var() / K + ref_v.sum() / 4096), (tg.mean(), tr)
    assert ref_m.mean() > 0.02                                 # the point emitter and the environment both reach the film
    # transient: optical path lengths binned into 1-unit frames
    F = 20
    ref_m, _, ref_f, ref_fv = vp.render(mf.Distr(kind, alpha, visible), spp=2048, seed=2, cam_to_world=p.cam_to_world, frames=(0.0, 1.0, F))
    p.decomposition = P.DECOMPOSITION_TRANSIENT; p.min_bound = 0.0; p.max_bound = float(F); p.bin_width = 1.0
    sc, _ = ctx.upload_scene(p)
    tot = []
    for b in range(8):
        f = ctx.render_to_host(sc, 0, 128, seed=100 + b)
        tot.append([(f[..., 3 * k] / f[..., -1]).sum() for k in range(F)])
    tot = np.array(tot)
    zf = (tot.mean(0) - ref_f) / np.sqrt(tot.var(0) / 8 + ref_fv + 1e-12)
    assert np.all(np.abs(zf) < 4.5), (zf.round(2), tot.mean(0).round(3), ref_f.round(3))
    assert abs(tot.mean(0).sum() - ref_m.sum()) < 0.02 * ref_m.sum()          # the frames hold the whole image


@pytest.mark.parametrize("kind,alpha,visible", [(P.MICROFACET_GGX, 0.25, True), (P.MICROFACET_BECKMANN, 0.15, True), (P.MICROFACET_PHONG, 0.3, False)])
def test_glossy_highlight_closed_form(ctx, kind, alpha, visible):
    """black environment, max_depth = 2: only the first surface vertex samples the emitter.  Per pixel, the float64 mean of
    I / r^2 eval(wi, wo) (exterior side) over a 24 x 24 grid of the pixel footprint (tests/ref64.pinhole_rays, the cube's face normal)"""
    from tests import ref64
    p = _cube_scene(kind, alpha, visible, env_radiance=[0.0] * 3, max_depth=2, w=24, h=24)
    m = 24
    g = (np.arange(m) + 0.5) / m
    py, px, sy, sx = np.meshgrid(np.arange(24), np.arange(24), g, g, indexing="ij")
    pos = np.stack([(px + sx).ravel(), (py + sy).ravel()], 1)
    o, d = ref64.pinhole_rays(p.cam_to_world, 24, 24, 50.0, pos)
    with np.errstate(divide="ignore", invalid="ignore"):
        t1 = (-1 - o) / d; t2 = (1 - o) / d
    tn = np.max(np.minimum(t1, t2), 1); tf = np.min(np.maximum(t1, t2), 1)
    hit = (tn <= tf) & (tf > 0)
    x = o + d * tn[:, None]
    k = np.argmax(np.abs(x), 1); n = np.zeros_like(x); n[np.arange(len(x)), k] = np.sign(x[np.arange(len(x)), k])
    val = np.zeros(len(x))
    for face in np.unique(k * 2 + (n[np.arange(len(x)), k] > 0)):
        sel = hit & (k * 2 + (n[np.arange(len(x)), k] > 0) == face)
        if not sel.any():
            continue
        s, t = mf.frame(n[sel][0])
        nn = n[sel][0]
        loc = lambda v: np.stack([v @ s, v @ t, v @ nn], 1)
        de = np.array(p.point_position) - x[sel]; r = np.linalg.norm(de, axis=1); de /= r[:, None]
        wl = loc(de)
        f, _ = mf.eval_pdf(mf.Distr(kind, alpha, visible), 1.5, loc(-d[sel]), wl)
        val[sel] = np.where(wl[:, 2] > 0, 3.0 * f / (r * r), 0.0)
    val = val.reshape(24, 24, m * m)
    ref, rvar = val.mean(-1), val.var(-1)
    sc, _ = ctx.upload_scene(p)
    spp = 1024
    film = ctx.render_to_host(sc, 0, spp, seed=5)
    gpu = film[..., 0] / film[..., 4]
    z = (gpu - ref) / np.sqrt(rvar / spp + 1e-14)
    assert ref.max() > 0.05                                    # a highlight is in view
    assert (np.abs(z) > 4.5).sum() <= 1 + 0.01 * z.size, (np.abs(z).max(), (np.abs(z) > 4.5).sum())
    assert abs(gpu.sum() - ref.sum()) < 4.5 * np.sqrt(rvar.sum() / spp) + 1e-3 * ref.sum(), (gpu.sum(), ref.sum())
