"""The HIP leaf kernels against float64 closed forms (tests/ref64.py), not against the oracle: the same checks tests/test_ref64.py proves
on the CPU oracle (tests/closed_form.py), at the edges where kernels go wrong -- step sizes and record layouts of the eikonal trace,
the spline near its limits, |g| near 1 and around Epsilon, the Bessel field on its axis and near its zeros, pixel corners."""
import numpy as np
import pytest
from mitsubaer_amd import capi, params as P
from tests import closed_form as cf, hg_ref, ref64, scenes

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def be(ctx):
    return cf.Gpu(ctx)


LAYOUTS = {"dense": capi.LAYOUT_DENSE, "cell8": capi.LAYOUT_CELL8, "brick27": capi.LAYOUT_BRICK27}


# RK4's 1/n is v_rcp_f32 (<= 1 ulp) and the oracle's fp32 error against the closed form is <= 5e-7: 4e-6 allows 8x that
@pytest.mark.parametrize("field", cf.LINEAR_FIELDS, ids=["b0.15", "b0.45"])
@pytest.mark.parametrize("stepper", [P.STEP_RK4, P.STEP_VERLET], ids=["rk4", "verlet"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_trace_in_a_linear_index_against_the_exact_ray(be, field, stepper, layout):
    cf.check_linear_trace(be, *field, stepper, layout=LAYOUTS[layout], tol=4e-6)


@pytest.mark.parametrize("stepper", [P.STEP_RK4, P.STEP_VERLET], ids=["rk4", "verlet"])
def test_bspline_trace_in_a_linear_index_against_the_exact_ray(be, stepper):
    cf.check_linear_trace(be, *cf.LINEAR_FIELDS[1], stepper, kind="bspline", tol=8e-6)


def test_bouguer_radial_field(be):
    cf.check_bouguer(be)


def _spline_case(ctx, data, mn, mx, to_world=None):
    vol = ctx.upload_volume(data, mn, mx, to_world=to_world).build_spline()
    return vol, vol.download_spline()


def test_bspline_prefilter_interpolates_and_evaluator_matches_float64(ctx):
    """K_prefilter: the float64 spline of the downloaded coefficients passes through the data at every node inside the limits.
    The evaluator apart from the prefilter: the GPU value / gradient equal the float64 evaluation of the same coefficients at random
    points, points within 1e-3 stride of lim_min / lim_max and integer grid coordinates."""
    rng = np.random.RandomState(3)
    shape = (17, 20, 33); mn, mx = [-1, -2, 0], [1, 2, 3]
    data = (1.3 + 0.3 * rng.rand(*shape)).astype(np.float32)
    vol, coeff = _spline_case(ctx, data, mn, mx)
    st = np.array([(mx[i] - mn[i]) / (shape[2 - i] - 1) for i in range(3)])
    idx = np.array([[i, j, k] for k in range(3, shape[0] - 3) for j in range(3, shape[1] - 3) for i in range(3, shape[2] - 3)])
    nodes = np.array(mn) + idx * st
    v, _ = ref64.bspline_value_grad(coeff, mn, mx, nodes)
    assert np.abs(v - data[idx[:, 2], idx[:, 1], idx[:, 0]]).max() < 4e-6            # fp32 recursion of coefficients ~1.5
    lo = np.array(mn) + 2 * st; hi = np.array(mx) - 2 * st
    q = np.concatenate([rng.uniform(lo, hi, (20000, 3)), lo + 1e-3 * st * rng.rand(500, 3),
                        hi - 1e-3 * st * rng.rand(500, 3), nodes]).astype(np.float32)
    gv, gg = ctx.rif_value_grad(vol, P.RIF_BSPLINE3, q)
    rv, rg = ref64.bspline_value_grad(coeff, mn, mx, q.astype(np.float64))
    assert np.abs(gv - rv).max() < 2e-6
    assert np.abs(gg - rg).max() < 4e-5                                                 # fp32 sums of O(1) data times dxres ~ 10
    gv, _ = ctx.rif_value_grad(vol, P.RIF_BSPLINE3, nodes.astype(np.float32))
    assert np.abs(gv - data[idx[:, 2], idx[:, 1], idx[:, 0]]).max() < 6e-6
    vol.destroy()


def test_bspline_reproduces_a_linear_field(ctx):
    """linear data: value and gradient exact where the mirror boundary's term has died out (>= 6 strides from the box), and at every
    point inside the limits (down to 1e-3 stride from them) equal to the float64 spline of the downloaded coefficients -- there the
    prefilter's mirror boundary bends the field by (2 - sqrt 3)^k per node, which is the reference's own spline (basisspline.h)"""
    shape = (14, 21, 17); mn, mx = [-1, -2, 0], [1, 2, 3]
    ax = [np.linspace(mn[i], mx[i], shape[2 - i]) for i in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    gl = np.array([0.1, -0.05, 0.02])
    vol, coeff = _spline_case(ctx, (1.4 + gl[0] * x + gl[1] * y + gl[2] * z).astype(np.float32), mn, mx)
    st = np.array([(mx[i] - mn[i]) / (shape[2 - i] - 1) for i in range(3)])
    rng = np.random.RandomState(1)
    inner = rng.uniform(np.array(mn) + 6 * st, np.array(mx) - 6 * st, (4000, 3)).astype(np.float32)
    v, g = ctx.rif_value_grad(vol, P.RIF_BSPLINE3, inner)
    assert np.abs(v - (1.4 + inner.astype(np.float64) @ gl)).max() < 6e-6 and np.abs(g - gl).max() < 6e-5
    lo = np.array(mn) + 2 * st; hi = np.array(mx) - 2 * st
    edge = np.concatenate([lo + 1e-3 * st * rng.rand(1000, 3), hi - 1e-3 * st * rng.rand(1000, 3)]).astype(np.float32)
    v, g = ctx.rif_value_grad(vol, P.RIF_BSPLINE3, edge)
    rv, rg = ref64.bspline_value_grad(coeff, mn, mx, edge.astype(np.float64))
    assert np.abs(v - rv).max() < 2e-6 and np.abs(g - rg).max() < 2e-5
    vol.destroy()


def test_bspline_under_a_rotated_data_box(ctx):
    """toWorld: the float64 spline evaluated at worldToVolume(p), its gradient rotated back (splinevolume.cpp:343,359)"""
    N = 20
    tw = P.rotation([1, 2, 3], 35.0, [0.1, 0.0, -0.05])
    rng = np.random.RandomState(4)
    data = (1.4 + 0.1 * rng.rand(N, N, N)).astype(np.float32)
    mn, mx = [-1.3] * 3, [1.3] * 3
    vol, coeff = _spline_case(ctx, data, mn, mx, to_world=tw)
    pts = scenes.rand_points(8000, -0.5, 0.5, seed=3)                      # inside the limits after the rotation and shift
    gv, gg = ctx.rif_value_grad(vol, P.RIF_BSPLINE3, pts)
    M = np.linalg.inv(np.asarray(tw, np.float64))
    q = pts.astype(np.float64) @ M[:3, :3].T + M[:3, 3]
    rv, rg = ref64.bspline_value_grad(coeff, mn, mx, q)
    rg = rg @ M[:3, :3]
    assert np.abs(gv - rv).max() < 2e-6 and np.abs(gg - rg).max() < 2e-5
    vol.destroy()


@pytest.mark.parametrize("g", hg_ref.G_EDGES)
def test_hg_at_the_edges_of_g(ctx, g):
    g32 = float(np.float32(g))
    hg_ref.check_hg(lambda wi, u2: ctx.phase_sample(P.PHASE_HG, g32, wi, u2), lambda wi, wo: ctx.phase_eval(P.PHASE_HG, g32, wi, wo), g)


@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_acoustic_rif_against_the_float64_bessel_reference(be, m):
    """J_m (series below 1, jnf above) / atan2f / cosf on the device against the trapezoid Bessel reference: 4e-6 of n_max (the
    oracle's fp32 error with glibc is below 1.2e-6), on the axis clamp and near zeros of J_m"""
    cf.check_acoustic(be, m, 4e-6)


def test_acoustic_entry_point_needs_the_acoustic_field(ctx):
    sc, vols = ctx.upload_scene(scenes.curved_scene(N=8))
    with pytest.raises(capi.MerError, match="acoustic"):
        ctx.acoustic_value_grad(sc, np.zeros((4, 3), np.float32))
    for v in vols:
        v.destroy()


def test_transmittance_and_free_flight(be):
    cf.check_transmittance(be)


@pytest.mark.parametrize("cam", cf.CAMERAS, ids=lambda c: "%dx%d_fov%g" % c)
def test_camera_rays_are_the_pinhole(be, cam):
    cf.check_camera(be, *cam)


def test_emission_only_slab_per_pixel(be):
    cf.check_emission_slab(be)


def test_point_emitter_single_scatter_matches_quadrature(be):
    cf.check_point_single_scatter(be)


def test_point_emitter_single_scatter_transient_profile(be):
    cf.check_point_single_scatter_transient(be)


def test_point_emitter_curved_equals_straight_in_constant_index(be):
    cf.check_point_curved_equals_straight(be)


def test_connection_in_a_constant_index_is_the_chord(ctx):
    """A12: in a constant index the connecting ray is the chord: arc length |p2 - p1|, optical length n |p2 - p1|, direction along it"""
    N = 12
    p = scenes.curved_scene(N=N, rif=np.full((N, N, N), 1.3, np.float32))
    sc, vols = ctx.upload_scene(p)
    rng = np.random.RandomState(5)
    p1 = rng.uniform(-0.8, 0.8, (256, 3)).astype(np.float32); p2 = rng.uniform(-0.8, 0.8, (256, 3)).astype(np.float32)
    out = ctx.connect(sc, p1, p2, 9)
    ok = out[:, 0] == 1
    assert ok.mean() > 0.85
    chord = (p2 - p1).astype(np.float64)[ok]; L = np.linalg.norm(chord, axis=1)
    w = out[ok, 1]                                                           # 1, or 1 / 0.01 after a Russian-roulette restart
    assert np.isin(w, [1.0, 100.0]).all() and (w == 1.0).mean() > 0.95
    np.testing.assert_allclose(out[ok, 8], L, rtol=2e-3)                     # arc length, quantised by the step size
    np.testing.assert_allclose(out[ok, 9], 1.3 * L, rtol=2e-3)
    d = out[ok, 2:5] / np.linalg.norm(out[ok, 2:5], axis=1, keepdims=True)
    np.testing.assert_allclose(d, chord / L[:, None], atol=2e-4)
    for v in vols:
        v.destroy()


# ---- curved free flights, connections and NEE against exact rays of n = 1.5 + 0.45 y: the deterministic bounds are 8 x the fp32 CPU
# oracle's measured deviation (closed_form.FREE_FLIGHT_MEASURED / CONNECT_MEASURED), never a GPU figure
@pytest.mark.parametrize("stepper", [P.STEP_RK4, P.STEP_VERLET], ids=["rk4", "verlet"])
def test_curved_transmittance_against_the_exact_ray(be, stepper):
    cf.check_curved_transmittance(be, stepper)


@pytest.mark.parametrize("ray", [0, 1])
@pytest.mark.parametrize("stepper", [P.STEP_RK4, P.STEP_VERLET], ids=["rk4", "verlet"])
@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_curved_free_flight_against_the_exact_ray(be, stepper, ray, layout):
    cf.check_curved_free_flight(be, stepper, ray, layout=LAYOUTS[layout], tol=8.0)


@pytest.mark.parametrize("layout", sorted(LAYOUTS))
def test_connection_in_a_linear_index_against_the_exact_ray(be, layout):
    cf.check_linear_connection(be, layout=LAYOUTS[layout], tol=8.0)


@pytest.mark.parametrize("gridded", [False, True], ids=["homogeneous", "gridded"])
def test_point_emitter_single_scatter_through_curved_rays(be, gridded):
    cf.check_point_single_scatter_curved(be, gridded)
