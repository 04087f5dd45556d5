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
