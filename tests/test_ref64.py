"""The float64 closed forms of tests/ref64.py proved against the CPU oracle, fp32 and fp64 (rif_double = 1), before any GPU sees them:
this pins the oracle from outside, and the same checks (tests/closed_form.py) then hold the HIP kernels to the same truths
(tests/test_gpu_closed_form.py).  CPU only."""
import numpy as np
import pytest
from mitsubaer_amd import params as P, synth
from tests import closed_form as cf, hg_ref, ref64


@pytest.fixture(scope="module", params=[False, True], ids=["fp32", "fp64"])
def be(orc, request):
    return cf.Oracle(orc, double=request.param)


@pytest.mark.parametrize("field", cf.LINEAR_FIELDS, ids=["b0.15", "b0.45"])
@pytest.mark.parametrize("stepper", [P.STEP_RK4, P.STEP_VERLET], ids=["rk4", "verlet"])
def test_trace_in_a_linear_index_against_the_exact_ray(be, field, stepper):
    cf.check_linear_trace(be, *field, stepper)


@pytest.mark.parametrize("stepper", [P.STEP_RK4, P.STEP_VERLET], ids=["rk4", "verlet"])
def test_bspline_trace_in_a_linear_index_against_the_exact_ray(be, stepper):
    cf.check_linear_trace(be, *cf.LINEAR_FIELDS[1], stepper, kind="bspline", tol=5e-6)


def test_verlet_order_continues_to_small_steps(orc):
    """first order all the way down (0.3 -> 0.01875): the reference's er_step, not a second-order Verlet"""
    cf.check_linear_trace(cf.Oracle(orc, True), *cf.LINEAR_FIELDS[1], P.STEP_VERLET, hs=(0.3, 0.15, 0.075, 0.0375, 0.01875))


def test_bouguer_radial_field(be):
    cf.check_bouguer(be)


def test_closed_form_trajectory_is_a_solution():
    """the reference itself: finite differences of the closed form satisfy dp/ds = v/n and dv/ds = grad n, and |v| = n(p)"""
    a, b = 1.5, 0.45
    p0 = np.array([[0.1, -0.2, 0.3], [0.0, 0.25, -0.1]]); d0 = np.array([[0.3, 0.8, -0.2], [0.5, -0.7, 0.4]])
    s, e = 0.37, 1e-6
    p, v, o = ref64.linear_index_trajectory(a, b, p0, d0, s)
    pp, vp, op = ref64.linear_index_trajectory(a, b, p0, d0, s + e)
    pm, vm, om = ref64.linear_index_trajectory(a, b, p0, d0, s - e)
    n = a + b * p[:, 1]
    assert np.abs((pp - pm) / (2 * e) - v / n[:, None]).max() < 1e-7
    assert np.abs((vp - vm) / (2 * e) - [0, b, 0]).max() < 1e-7
    assert np.abs((op - om) / (2 * e) - n).max() < 1e-7
    assert np.abs(np.linalg.norm(v, axis=1) - n).max() < 1e-12


def test_bspline_reference_on_the_oracle_coefficients(orc):
    """ref64's evaluator on the oracle's coefficients: interpolation at every node inside the limits; equal to the oracle's own
    evaluation (fp64 to round-off, fp32 to its rounding), also within 1e-3 stride of the limits; a linear field reproduced exactly where
    the mirror boundary's term (decaying as (2 - sqrt 3)^k per node) has died out"""
    rng = np.random.RandomState(0)
    shape = (14, 21, 17); mn, mx = [-1, -2, 0], [1, 2, 3]
    st = np.array([(mx[i] - mn[i]) / (shape[2 - i] - 1) for i in range(3)])
    data = rng.rand(*shape).astype(np.float32)
    c64 = orc.bspline_build(data, double=True)
    idx = np.array([[i, j, k] for k in range(3, shape[0] - 3) for j in range(3, shape[1] - 3) for i in range(3, shape[2] - 3)])
    v, _ = ref64.bspline_value_grad(c64, mn, mx, np.array(mn) + idx * st)
    assert np.abs(v - data[idx[:, 2], idx[:, 1], idx[:, 0]]).max() < 1e-12
    lo = np.array(mn) + 2 * st; hi = np.array(mx) - 2 * st
    q = np.concatenate([rng.uniform(lo, hi, (3000, 3)), lo + 1e-3 * st * rng.rand(200, 3), hi - 1e-3 * st * rng.rand(200, 3)])
    rv, rg = ref64.bspline_value_grad(c64, mn, mx, q)
    ov, og = orc.bspline_eval(c64, mn, mx, q)
    assert np.abs(ov - rv).max() < 1e-13 and np.abs(og - rg).max() < 1e-12
    c32 = orc.bspline_build(data)
    q32 = q.astype(np.float32)
    rv, rg = ref64.bspline_value_grad(c32, mn, mx, q32)
    ov, og = orc.bspline_eval(c32, mn, mx, q32)
    assert np.abs(ov - rv).max() < 2e-6 and np.abs(og - rg).max() < 4e-5         # fp32 sums of O(1) data times dxres ~ 8
    ax = [np.linspace(mn[i], mx[i], shape[2 - i]) for i in range(3)]
    z, y, x = np.meshgrid(ax[2], ax[1], ax[0], indexing="ij")
    lin = (1.4 + 0.1 * x - 0.05 * y + 0.02 * z)
    c = orc.bspline_build(lin.astype(np.float32), double=True)
    inner = rng.uniform(np.array(mn) + 6 * st, np.array(mx) - 6 * st, (500, 3))
    v, g = ref64.bspline_value_grad(c, mn, mx, inner)
    assert np.abs(v - (1.4 + inner @ [0.1, -0.05, 0.02])).max() < 5e-6 and np.abs(g - [0.1, -0.05, 0.02]).max() < 5e-5


@pytest.mark.parametrize("g", hg_ref.G_EDGES)
def test_hg_at_the_edges_of_g(orc, g):
    g32 = float(np.float32(g))
    hg_ref.check_hg(lambda wi, u2: orc.phase_sample(P.PHASE_HG, g32, wi, u2), lambda wi, wo: orc.phase_eval(P.PHASE_HG, g32, wi, wo), g)


def test_hg_reference_is_a_distribution():
    """hg_cdf is the integral of 2 pi hg_pdf (central differences), runs from 0 to 1, and hg_inverse_cdf inverts it"""
    for g in (0.999, -0.999, 0.99, 0.3, -0.3, 2e-4, 9.9e-5):
        mu = np.linspace(-1 + 1e-4, 1 - 1e-4, 2001)
        e = 1e-8 if abs(g) > 0.5 else 1e-5                # truncation near a sharp peak vs cancellation at small g
        dF = (ref64.hg_cdf(g, mu + e) - ref64.hg_cdf(g, mu - e)) / (2 * e)
        assert np.abs(dF / (2 * np.pi * ref64.hg_pdf(g, mu)) - 1).max() < 2e-4, g
        assert abs(ref64.hg_cdf(g, -1.0)) < 1e-10 and abs(ref64.hg_cdf(g, 1.0) - 1) < 1e-9
        u = np.linspace(0, 1, 101)
        assert np.abs(ref64.hg_cdf(g, ref64.hg_inverse_cdf(g, u)) - u).max() < 1e-8, g


def test_bessel_reference():
    """the trapezoid J_m against values of J_m tabulated to 10 digits (Abramowitz & Stegun table 9.1) and the recurrence"""
    table = {(0, 1.0): 0.7651976866, (1, 1.0): 0.4400505857, (2, 1.0): 0.1149034849, (0, 5.0): -0.1775967713, (1, 5.0): -0.3275791376,
             (3, 5.0): 0.3648312306, (0, 2.404825557695773): 0.0}
    for (m, x), want in table.items():
        assert abs(ref64.bessel_j(m, x) - want) < 1e-10, (m, x)
    x = np.linspace(0.1, 15, 300)
    for m in (1, 2, 3):
        assert np.abs(ref64.bessel_j(m - 1, x) + ref64.bessel_j(m + 1, x) - 2 * m / x * ref64.bessel_j(m, x)).max() < 1e-12


@pytest.mark.parametrize("m", [0, 1, 2, 3])
def test_acoustic_rif_against_the_float64_bessel_reference(be, m):
    cf.check_acoustic(be, m, 1e-8 if be.double else 4e-6)


def test_transmittance_and_free_flight(orc):
    cf.check_transmittance(cf.Oracle(orc))


@pytest.mark.parametrize("cam", cf.CAMERAS, ids=lambda c: "%dx%d_fov%g" % c)
def test_camera_rays_are_the_pinhole(orc, cam):
    cf.check_camera(cf.Oracle(orc), *cam)


def test_emission_only_slab_per_pixel(orc):
    cf.check_emission_slab(cf.Oracle(orc))


# ---- curved free flights, connections and NEE against exact rays of n = 1.5 + 0.45 y (CPU seconds: fp32 / fp64 alike)
def test_linear_index_connection_is_a_ray_between_its_points():
    """the connection reference itself: reversible (same arc and optical length, arrival = -launch of the reverse), a vertical pair is its
    chord with optical length mean(n) x length, the arc exceeds the chord and the optical length undercuts the chord's (the landing test runs inside the function)"""
    a, b = cf.CURVED_A, cf.CURVED_B
    rng = np.random.RandomState(2)
    p1 = rng.uniform(-0.7, 0.7, (256, 3)); p2 = rng.uniform(-0.7, 0.7, (256, 3))
    p1[0] = [0.1, -0.3, 0.2]; p2[0] = [0.1, 0.5, 0.2]
    v0, ve, arc, opt = ref64.linear_index_connection(a, b, p1, p2)
    r0, re, rarc, ropt = ref64.linear_index_connection(a, b, p2, p1)
    assert np.abs(arc - rarc).max() < 1e-12 and np.abs(opt - ropt).max() < 1e-12 and np.abs(ve + r0).max() < 1e-12 and np.abs(v0 + re).max() < 1e-12
    assert np.abs(np.linalg.norm(v0, axis=1) - (a + b * p1[:, 1])).max() < 1e-12 and np.abs(np.linalg.norm(ve, axis=1) - (a + b * p2[:, 1])).max() < 1e-12
    assert abs(arc[0] - 0.8) < 1e-12 and abs(opt[0] - (a + b * 0.1) * 0.8) < 1e-12
    L = np.linalg.norm(p2 - p1, axis=1)
    assert (arc - L).min() > -1e-12 and (arc - L).max() > 0.01 and np.all(opt <= (a + b * 0.5 * (p1[:, 1] + p2[:, 1])) * L + 1e-12)   # Fermat: no longer than the chord's optical length


def test_curve_optical_depth_quadrature_error():
    """halving the spacing: the quadrature of the gridded sigma_t along both exact rays has converged to 1e-7 at the table the checks use
    (tau ~ 2.3 and 3.2; the Monte Carlo standard errors it is compared with are above 1e-3 of tau), and tau is increasing up to the exit"""
    p = cf.curved_case()
    for i in range(len(cf.CURVED_RAYS)):
        s, tau, sx = cf._curved_tau(p, i)
        s2, tau2, sx2 = cf._curved_tau(p, i, m=2 * (len(s) - 1) + 1)
        s4, tau4, _ = cf._curved_tau(p, i, m=(len(s) - 1) // 2 + 1)
        assert sx == sx2 and abs(tau[-1] - tau2[-1]) < 1e-7 and abs(tau4[-1] - tau[-1]) < 4e-7, (tau4[-1], tau[-1], tau2[-1])
        assert np.abs(np.interp(s[::50], s2, tau2) - tau[::50]).max() < 1e-7
        assert np.all(np.diff(tau) >= 0) and np.all(np.diff(s) > 0)
        end, _, _ = ref64.linear_index_trajectory(cf.CURVED_A, cf.CURVED_B, [cf.CURVED_RAYS[i][0]], [cf.CURVED_RAYS[i][1]], sx)
        assert abs(np.abs(end).max() - 1) < 1e-6                                    # the table ends on a face of the cube
    # a constant sigma_t: tau = sigma_t x arc
    s, tau, sx = ref64.curve_optical_depth(cf.CURVED_A, cf.CURVED_B, None, 1.0, [-0.6, 0.5, -0.3], [1.0, 0.3, 0.2], sigma_t=1.2)
    assert np.abs(tau - 1.2 * s).max() < 1e-9


def test_curved_single_scatter_quadrature_error():
    """halving both spacings moves the quadrature of check_point_single_scatter_curved by less than 1e-4 of itself (the check allows 3 %),
    and with b -> 0 it is the straight-ray quadrature of point_single_scatter times the phase function"""
    for gridded in (False, True):
        p = cf.curved_single_scatter_scene(gridded)
        ref = cf.curved_single_scatter_reference(p, gridded)[0]
        kw = dict(density=p.density, scale=p.density_scale, albedo=p.albedo[0]) if gridded else dict(sigma_t=1.2, albedo=0.75)
        half = ref64.point_single_scatter_curved(cf.CURVED_A, cf.CURVED_B, [-1, 0, 0], [1, 0, 0], p.point_position, p.g, n=801, m=401, **kw)[0]
        assert abs(half / ref - 1) < 1e-4, (half, ref)
    flat = ref64.point_single_scatter_curved(1.3, 1e-5, [-1, 0, 0], [1, 0, 0], [0.1, 0.6, -0.2], 0.0, 0.75, sigma_t=1.2)[0]
    straight = ref64.point_single_scatter([-3, 0, 0], [1, 0, 0], 2.0, 4.0, 0.3, 0.9, [0.1, 0.6, -0.2])[0]
    assert abs(flat / straight - 1) < 1e-4, (flat, straight)


@pytest.mark.parametrize("stepper", [P.STEP_RK4, P.STEP_VERLET], ids=["rk4", "verlet"])
def test_curved_transmittance_against_the_exact_ray(be, stepper):
    """1 s (RK4), 9 s (Verlet at the small step)"""
    cf.check_curved_transmittance(be, stepper)


@pytest.mark.parametrize("ray", [0, 1])
@pytest.mark.parametrize("stepper", [P.STEP_RK4, P.STEP_VERLET], ids=["rk4", "verlet"])
def test_curved_free_flight_against_the_exact_ray(be, stepper, ray):
    """1 s (RK4), 4 s (Verlet)"""
    cf.check_curved_free_flight(be, stepper, ray)


def test_connection_in_a_linear_index_against_the_exact_ray(be):
    """3 s: 512 pairs in 0.1 s, the rest is the 3 x 200 000 seeds of the expectation"""
    cf.check_linear_connection(be)


@pytest.mark.parametrize("gridded", [False, True], ids=["homogeneous", "gridded"])
def test_point_emitter_single_scatter_through_curved_rays(orc, gridded):
    """42 s / 62 s on 8 threads: sized by the weight-100 restarts; fp32 only"""
    cf.check_point_single_scatter_curved(cf.Oracle(orc), gridded)
