"""Float64 closed forms and quadratures for the leaf operations: ground truth that depends on neither the HIP kernels nor the
CPU oracle.  numpy only.  Conventions (axis order, wi pointing away from the vertex, [z][y][x] arrays) follow mitsubaer_amd."""
import numpy as np

INV_FOURPI = 1.0 / (4.0 * np.pi)


# ------------------------------------------------------------------------------------ eikonal ray in n = a + b y
def linear_index_trajectory(a, b, p0, d0, s):
    """Exact ray of the eikonal equation dp/ds = v/n, dv/ds = grad n in the index n(p) = a + b p_y, started at p0 with unit
    direction d0 (v0 = n(p0) d0) and followed for arc length s.  With ds = n dsigma and u = n: u'' = b^2 u, so
    u = u0 cosh(b sigma) + v_y0 sinh(b sigma), v_y = u0 sinh + v_y0 cosh, x and z linear in sigma; arc length
    s(sigma) = (u0 sinh + v_y0 (cosh - 1)) / b is increasing and is inverted by bisection; optical length = int u^2 dsigma.
    Returns (p[n,3], v[n,3], optical_length[n])."""
    p0 = np.asarray(p0, np.float64); d0 = np.asarray(d0, np.float64)
    d0 = d0 / np.linalg.norm(d0, axis=1, keepdims=True)
    s = np.broadcast_to(np.asarray(s, np.float64), p0.shape[:1])
    u0 = a + b * p0[:, 1]
    v0 = d0 * u0[:, None]

    def arc(sig):
        return (u0 * np.sinh(b * sig) + v0[:, 1] * (np.cosh(b * sig) - 1.0)) / b

    lo = np.zeros_like(s); hi = s / np.maximum(u0, 1e-3) * 4.0 + 1e-3
    while np.any(arc(hi) < s):
        hi = np.where(arc(hi) < s, 2.0 * hi, hi)
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        below = arc(mid) < s
        lo = np.where(below, mid, lo); hi = np.where(below, hi, mid)
    sig = 0.5 * (lo + hi)
    ch, sh = np.cosh(b * sig), np.sinh(b * sig)
    u = u0 * ch + v0[:, 1] * sh
    p = np.stack([p0[:, 0] + v0[:, 0] * sig, (u - a) / b, p0[:, 2] + v0[:, 2] * sig], 1)
    v = np.stack([v0[:, 0], u0 * sh + v0[:, 1] * ch, v0[:, 2]], 1)
    # int (A cosh + B sinh)^2: A^2 (sig/2 + sinh 2b sig / 4b) + 2AB (cosh 2b sig - 1) / 4b + B^2 (sinh 2b sig / 4b - sig/2)
    A, B = u0, v0[:, 1]
    s2, c2 = np.sinh(2 * b * sig), np.cosh(2 * b * sig)
    opt = A * A * (sig / 2 + s2 / (4 * b)) + 2 * A * B * (c2 - 1) / (4 * b) + B * B * (s2 / (4 * b) - sig / 2)
    return p, v, opt


def _linear_index_at_sigma(a, b, p0, v0, sig):
    """the same ray at the parameter sigma (ds = n dsigma) instead of at an arc length: (p, v, arc, optical_length), no inversion.
    p0, v0 [n,3]; sig [n] or [n,m] (then p, v are [n,m,3])"""
    p0 = np.asarray(p0, np.float64); v0 = np.asarray(v0, np.float64); sig = np.asarray(sig, np.float64)
    ex = (slice(None),) + (None,) * (sig.ndim - 1)
    u0 = (a + b * p0[:, 1])[ex]; w0 = v0[:, 1][ex]
    ch, sh = np.cosh(b * sig), np.sinh(b * sig)
    u = u0 * ch + w0 * sh
    p = np.stack([p0[:, 0][ex] + v0[:, 0][ex] * sig, (u - a) / b, p0[:, 2][ex] + v0[:, 2][ex] * sig], -1)
    v = np.stack([v0[:, 0][ex] + 0 * sig, u0 * sh + w0 * ch, v0[:, 2][ex] + 0 * sig], -1)
    arc = (u0 * sh + w0 * (ch - 1.0)) / b
    s2, c2 = np.sinh(2 * b * sig), np.cosh(2 * b * sig)
    opt = u0 * u0 * (sig / 2 + s2 / (4 * b)) + 2 * u0 * w0 * (c2 - 1) / (4 * b) + w0 * w0 * (s2 / (4 * b) - sig / 2)
    return p, v, arc, opt


def linear_index_connection(a, b, p1, p2, with_sigma=False):
    """The exact eikonal ray from p1 to p2 in n = a + b y.  It lies in the plane through p1 spanned by e_y and the horizontal part w of
    p2 - p1 (the momentum's horizontal part is conserved), so one unknown remains, the launch elevation phi: with H the horizontal
    distance, the ray reaches the column of p2 at sigma = H / (n1 cos phi), and there n = n1 (cosh b sigma + sin phi sinh b sigma) must be
    n(p2).  Newton on phi from the chord's elevation: the root nearest the chord (the other family of roots are the rays that first dip
    through the turning point).  A vertical pair (H = 0) is its chord.
    Returns (v0[n,3] with |v0| = n(p1), v_arrival[n,3], arc[n], optical_length[n]); asserts that linear_index_trajectory from p1
    along v0 lands on p2 within 1e-9.  with_sigma adds the ray parameter at p2."""
    p1 = np.atleast_2d(np.asarray(p1, np.float64)); p2 = np.atleast_2d(np.asarray(p2, np.float64))
    dh = p2[:, [0, 2]] - p1[:, [0, 2]]
    H = np.linalg.norm(dh, axis=1)
    vert = H < 1e-12
    w = np.where(vert[:, None], [1.0, 0.0], dh / np.where(vert, 1.0, H)[:, None])
    n1, n2 = a + b * p1[:, 1], a + b * p2[:, 1]
    phi = np.arctan2(p2[:, 1] - p1[:, 1], H)
    chord = phi.copy()
    for _ in range(50):
        c, s_ = np.cos(phi), np.sin(phi)
        sig = H / (n1 * c)
        ch, sh = np.cosh(b * sig), np.sinh(b * sig)
        f = n1 * (ch + s_ * sh) - n2
        df = n1 * (b * (sh + s_ * ch) * sig * np.tan(phi) + c * sh)                  # d sigma / d phi = sigma tan phi
        phi = np.where(vert, phi, phi - f / np.where(df == 0, 1.0, df))
    assert np.all((np.abs(phi) < np.pi / 2) | vert) and np.abs(phi - chord).max() < 0.5, "linear_index_connection: Newton left the chord's root"
    c, s_ = np.cos(phi), np.sin(phi)
    d0 = np.stack([c * w[:, 0], s_, c * w[:, 1]], 1)
    v0 = d0 * n1[:, None]
    sig = np.where(vert, np.abs(np.log(n2 / n1) / b), H / (n1 * np.where(vert, 1.0, c)))        # vertical: n = n1 exp(+-b sigma)
    _, ve, arc, opt = _linear_index_at_sigma(a, b, p1, v0, sig)
    pe, _, _ = linear_index_trajectory(a, b, p1, d0, arc)
    assert np.abs(pe - p2).max() < 1e-9, np.abs(pe - p2).max()
    return (v0, ve, arc, opt, sig) if with_sigma else (v0, ve, arc, opt)


# ------------------------------------------------------------------------------------ gridded sigma_t along the exact ray
def trilinear_sigma(density, scale, pts):
    """scale x the trilinear interpolant of density[z][y][x] (nodes spanning [-1,1]^3) in float64, with lookupFloat's cell rule
    (gridvolume.cpp: cell = floor of the grid coordinate; 0 where the cell's lower node is below 0 or its upper node past the last)"""
    data = np.asarray(density, np.float64)
    pts = np.asarray(pts, np.float64)
    n = np.array(data.shape[::-1])
    g = (pts + 1.0) * (n - 1) / 2.0
    i = np.floor(g).astype(np.int64)
    ok = np.all((i >= 0) & (i + 1 < n), axis=-1)
    i = np.clip(i, 0, n - 2); f = g - i
    out = 0.0
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                wgt = (f[..., 0] if dx else 1 - f[..., 0]) * (f[..., 1] if dy else 1 - f[..., 1]) * (f[..., 2] if dz else 1 - f[..., 2])
                out = out + wgt * data[i[..., 2] + dz, i[..., 1] + dy, i[..., 0] + dx]
    return scale * np.where(ok, out, 0.0)


def _sigma_exit(a, b, p0, v0, hi=8.0):
    """the parameter sigma at which each ray leaves [-1,1]^3 (the start lies inside): first crossing on a coarse table, then bisection"""
    p0 = np.asarray(p0, np.float64)
    tab = np.linspace(0.0, hi, 4001)[None, :] / (a + b * p0[:, 1:2])
    p, _, _, _ = _linear_index_at_sigma(a, b, p0, v0, tab)
    out = np.any(np.abs(p) > 1.0, axis=-1)
    assert out[:, -1].all() and not out[:, 0].any()
    k = np.argmax(out, axis=1); r = np.arange(len(p0))
    lo, hi_ = tab[r, k - 1], tab[r, k]
    for _ in range(80):
        mid = 0.5 * (lo + hi_)
        pm, _, _, _ = _linear_index_at_sigma(a, b, p0, v0, mid)
        o = np.any(np.abs(pm) > 1.0, axis=-1)
        lo = np.where(o, lo, mid); hi_ = np.where(o, mid, hi_)
    return lo * (1.0 - 1e-12)           # strictly inside: on the face itself the grid coordinate rounds to the last node, where lookupFloat is 0


def curve_optical_depth(a, b, density, scale, p0, d0, m=40001, sigma_t=None, displace=None):
    """tau(s) = int_0^s sigma_t ds' along the exact ray of n = a + b y from p0 (inside [-1,1]^3) along d0, up to the exit from the cube;
    sigma_t = trilinear_sigma(density, scale, .), or the constant sigma_t when density is None.  Trapezoid rule on m points equally spaced
    in the ray's parameter sigma (ds = n dsigma): the integrand has kinks at the cell faces, so the rule is second order in the spacing
    with an error of (cells crossed) x (spacing)^2 x (jump of the slope) / 12, shown by halving in tests/test_ref64.py.
    displace(arc[m]) -> [m,3], if given, is added to the ray's points before sigma_t is looked up (the exit stays the exact ray's): the
    optical depth a stepper with a known position error would see.  Returns (s[m], tau[m], s_exit) for one ray."""
    p0 = np.asarray(p0, np.float64).reshape(1, 3); d0 = np.asarray(d0, np.float64).reshape(1, 3)
    v0 = d0 / np.linalg.norm(d0) * (a + b * p0[:, 1:2])
    sig = np.linspace(0.0, _sigma_exit(a, b, p0, v0)[0], m)[None, :]
    p, v, arc, _ = _linear_index_at_sigma(a, b, p0, v0, sig)
    q = p[0] if displace is None else p[0] + displace(arc[0])
    st = trilinear_sigma(density, scale, q) if density is not None else np.full(m, float(sigma_t))
    f = st * (a + b * p[0, :, 1])                                                   # sigma_t ds = sigma_t n dsigma
    tau = np.concatenate([[0.0], np.cumsum(0.5 * (f[1:] + f[:-1]) * np.diff(sig[0]))])
    return arc[0], tau, arc[0, -1]


# ------------------------------------------------------------------------------------ cubic B-spline
def _bspline_w(t):
    """uniform cubic B-spline weights and their derivatives at the four taps floor(x)-1 .. floor(x)+2, t = x - floor(x)"""
    w = np.stack([(1 - t) ** 3 / 6, 2.0 / 3 - t * t + 0.5 * t ** 3, 2.0 / 3 - (1 - t) ** 2 + 0.5 * (1 - t) ** 3, t ** 3 / 6], -1)
    dw = np.stack([-0.5 * (1 - t) ** 2, 1.5 * t * t - 2 * t, -(1.5 * (1 - t) ** 2 - 2 * (1 - t)), 0.5 * t * t], -1)
    return w, dw


def bspline_value_grad(coeff, xmin, xmax, pts):
    """value and world-space gradient of sum_ijk c[k,j,i] beta3(x - i) beta3(y - j) beta3(z - k), with grid coordinates
    x = (p - xmin) (N - 1) / (xmax - xmin).  coeff[z][y][x]; the point must lie where all 4^3 taps exist."""
    c = np.asarray(coeff, np.float64)
    pts = np.asarray(pts, np.float64)
    N = np.array([c.shape[2], c.shape[1], c.shape[0]])
    mn = np.asarray(xmin, np.float64); mx = np.asarray(xmax, np.float64)
    sc = (N - 1) / (mx - mn)
    g = (pts - mn) * sc
    fl = np.floor(g)
    i0 = fl.astype(np.int64) - 1
    if (i0 < 0).any() or (i0 + 3 >= N).any():
        raise ValueError("bspline_value_grad: a tap falls outside the coefficient array")
    W = []; D = []
    for a in range(3):
        w, dw = _bspline_w(g[:, a] - fl[:, a]); W.append(w); D.append(dw)
    ar = np.arange(4)
    ix = i0[:, 0:1] + ar; iy = i0[:, 1:2] + ar; iz = i0[:, 2:3] + ar
    C = c[iz[:, :, None, None], iy[:, None, :, None], ix[:, None, None, :]]           # [n][k][j][i]
    val = np.einsum("nkji,nk,nj,ni->n", C, W[2], W[1], W[0])
    gx = np.einsum("nkji,nk,nj,ni->n", C, W[2], W[1], D[0]) * sc[0]
    gy = np.einsum("nkji,nk,nj,ni->n", C, W[2], D[1], W[0]) * sc[1]
    gz = np.einsum("nkji,nk,nj,ni->n", C, D[2], W[1], W[0]) * sc[2]
    return val, np.stack([gx, gy, gz], 1)


# ------------------------------------------------------------------------------------ Henyey-Greenstein
def hg_pdf(g, cos_theta):
    """HG density over solid angle; cos_theta = cosine between the scattered direction and the propagation direction -wi"""
    mu = np.asarray(cos_theta, np.float64)
    t = 1 + g * g - 2 * g * mu
    return INV_FOURPI * (1 - g * g) / (t * np.sqrt(t))


def hg_cdf(g, mu):
    """P(cos theta <= mu); the isotropic limit for g = 0"""
    mu = np.asarray(mu, np.float64)
    if g == 0:
        return 0.5 * (mu + 1)
    return (1 - g * g) / (2 * g) * (1 / np.sqrt(1 + g * g - 2 * g * mu) - 1 / (1 + g))


def hg_inverse_cdf(g, u):
    """cos theta for the uniform number u (increasing in u): the exact inverse of hg_cdf"""
    u = np.asarray(u, np.float64)
    if g == 0:
        return 2 * u - 1
    sq = (1 - g * g) / (1 - g + 2 * g * u)
    return np.clip((1 + g * g - sq * sq) / (2 * g), -1.0, 1.0)


def hg_condition(g, cos_theta):
    """relative condition number of hg_pdf's t = 1 + g^2 - 2 g cos: (1 + g^2) / t -- the factor by which a float32 evaluation
    loses accuracy near the forward peak of a strongly peaked lobe"""
    t = 1 + g * g - 2 * g * np.asarray(cos_theta, np.float64)
    return (1 + g * g) / t


# ------------------------------------------------------------------------------------ Bessel functions and the acoustic RIF
def bessel_j(m, x):
    """J_m(x) = (1/pi) int_0^pi cos(m tau - x sin tau) d tau by the trapezoid rule (exponentially convergent: the integrand is the
    half period of a smooth periodic function); integer m >= 0, any real x"""
    x = np.asarray(x, np.float64)
    K = int(2 * (np.abs(x).max(initial=0.0) + m) + 64)
    tau = np.linspace(0.0, np.pi, K + 1)
    w = np.full(K + 1, 1.0 / K); w[0] = w[-1] = 0.5 / K
    return (np.cos(m * tau[None, :] - x.reshape(-1, 1) * np.sin(tau)[None, :]) @ w).reshape(x.shape)


def bessel_j_prime(m, x):
    """dJ_m/dx = (J_{m-1} - J_{m+1}) / 2, J_{-1} = -J_1"""
    jm1 = -bessel_j(1, x) if m == 0 else bessel_j(m - 1, x)
    return 0.5 * (jm1 - bessel_j(m + 1, x))


def acoustic_value_grad(n_o, n_max, k_r, m, pts, eps=1e-8):
    """n = n_o + n_max J_m(k_r r) cos(m phi), r = |(y, z)|, phi = atan2(y, z) (the x axis is the cylinder axis), and its gradient.
    Below r = eps the reference's valueAndGradient (acousticrifvolume.cpp:235-239) replaces y, z and r by eps after phi is taken:
    reproduced here, it is that plugin's definition of the field at the axis."""
    q = np.asarray(pts, np.float64)
    y, z = q[:, 1].copy(), q[:, 2].copy()
    r = np.hypot(y, z); phi = np.arctan2(y, z)
    small = r < eps
    y[small] = eps; z[small] = eps; r[small] = eps
    J = bessel_j(m, k_r * r); Jp = bessel_j_prime(m, k_r * r)
    cm, sm = np.cos(m * phi), np.sin(m * phi)
    val = n_o + n_max * J * cm
    gy = n_max * (k_r * Jp * y / r * cm - J * m * sm * z / (r * r))
    gz = n_max * (k_r * Jp * z / r * cm + J * m * sm * y / (r * r))
    return val, np.stack([np.zeros_like(gy), gy, gz], 1)


# ------------------------------------------------------------------------------------ transmittance and free flight
def linear_sigma_optical_depth(s0, s1, t):
    """int_0^t (s0 + s1 x) dx for an extinction that is linear along the ray"""
    t = np.asarray(t, np.float64)
    return s0 * t + 0.5 * s1 * t * t


def linear_sigma_transmittance(s0, s1, t):
    return np.exp(-linear_sigma_optical_depth(s0, s1, t))


def linear_sigma_free_flight_cdf(s0, s1, t):
    """P(collision before t) = 1 - exp(-int_0^t sigma_t)"""
    return -np.expm1(-linear_sigma_optical_depth(s0, s1, t))


# ------------------------------------------------------------------------------------ camera
def pinhole_rays(cam_to_world, width, height, fov_x_deg, pos):
    """perspective sensor ray through film position pos (pixels, origin at the top-left corner): with u = x/W, v = y/H and aspect
    W/H, the camera-space direction is (tan(fov_x/2) (1 - 2u), tan(fov_x/2) (1 - 2v) / aspect, 1) normalised; world = the
    camera-to-world rotation of it, origin = the camera position.  Returns (o[n,3], d[n,3])."""
    M = np.asarray(cam_to_world, np.float64)[:3, :4]
    pos = np.asarray(pos, np.float64)
    tx = np.tan(np.deg2rad(fov_x_deg) / 2)
    aspect = width / height
    dc = np.stack([tx * (1 - 2 * pos[:, 0] / width), tx * (1 - 2 * pos[:, 1] / height) / aspect, np.ones(len(pos))], 1)
    dc /= np.linalg.norm(dc, axis=1, keepdims=True)
    d = dc @ M[:, :3].T
    o = np.broadcast_to(M[:, 3], d.shape).copy()
    return o, d


def box_chord(o, d, bmin, bmax):
    """length of the segment of the ray o + t d (t >= 0, unit d) inside the box [bmin, bmax]"""
    o = np.asarray(o, np.float64); d = np.asarray(d, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        t0 = (np.asarray(bmin, np.float64) - o) / d; t1 = (np.asarray(bmax, np.float64) - o) / d
    tn = np.nanmax(np.minimum(t0, t1), axis=1); tf = np.nanmin(np.maximum(t0, t1), axis=1)
    return np.maximum(tf - np.maximum(tn, 0.0), 0.0)


# ------------------------------------------------------------------------------------ single scattering
def point_single_scatter_curved(a, b, p_in, d_in, point, g, albedo, density=None, scale=1.0, sigma_t=None, n=1601, m=801):
    """Radiance per unit intensity that one scattering of a point emitter's light sends back along a camera ray entering the cube at
    p_in with direction d_in, curved rays in n = a + b y ("point emitter ... curved rays (A12)" and "refractive hooks"):
      int  e^{-tau(s)}  sigma_s(x)  phase(arrival direction -> launch direction of the connection)  /  |q - x|^2      [point.cpp: straight-line distance]
           x  e^{-tau_connection}  x  (n(x) / n(p_in))^2  ds                                                           [edge.cpp:91-93: the free flight's refRatioSq; none for the connection]
    over the camera's exact ray x(s) up to its exit, sigma_s = albedo sigma_t, sigma_t gridded (density, scale) or the constant sigma_t,
    the connection being the exact ray x -> q (linear_index_connection) and tau_connection the integral of sigma_t over ITS arc.
    Trapezoid rule, n vertices along the camera ray and m points along each connection, both equally spaced in the ray parameter.
    Returns (total, s[n], integrand[n], bend[n]): bend = angle between the connection's launch direction and the chord."""
    p_in = np.asarray(p_in, np.float64).reshape(1, 3); d_in = np.asarray(d_in, np.float64).reshape(1, 3)
    q = np.asarray(point, np.float64)
    st = (lambda pts: trilinear_sigma(density, scale, pts)) if density is not None else (lambda pts: np.full(pts.shape[:-1], float(sigma_t)))
    v_in = d_in / np.linalg.norm(d_in) * (a + b * p_in[:, 1:2])
    sig = np.linspace(0.0, _sigma_exit(a, b, p_in, v_in)[0], n)[None, :]
    x, v, s, _ = _linear_index_at_sigma(a, b, p_in, v_in, sig)
    x, v, s = x[0], v[0], s[0]
    nx = a + b * x[:, 1]
    fc = st(x) * nx
    tau = np.concatenate([[0.0], np.cumsum(0.5 * (fc[1:] + fc[:-1]) * np.diff(sig[0]))])
    v0, _, _, _, sc = linear_index_connection(a, b, x, np.broadcast_to(q, x.shape), with_sigma=True)
    u = np.linspace(0.0, 1.0, m)[None, :] * sc[:, None]
    pc, _, _, _ = _linear_index_at_sigma(a, b, x, v0, u)
    fk = st(pc) * (a + b * pc[..., 1])
    tau_c = (0.5 * (fk[:, 1:] + fk[:, :-1]) * np.diff(u, axis=1)).sum(1)
    chord = q[None] - x; r = np.linalg.norm(chord, axis=1)
    launch = v0 / np.linalg.norm(v0, axis=1, keepdims=True)
    cos = np.einsum("ij,ij->i", v / np.linalg.norm(v, axis=1, keepdims=True), launch)
    f = np.exp(-tau) * albedo * st(x) * hg_pdf(g, cos) / (r * r) * np.exp(-tau_c) * (nx / nx[0]) ** 2
    total = (0.5 * (f[1:] + f[:-1]) * np.diff(s)).sum()
    bend = np.arccos(np.clip(np.einsum("ij,ij->i", launch, chord / r[:, None]), -1, 1))
    return total, s, f, bend


def point_single_scatter(o, d, t_enter, t_exit, sigma_a, sigma_s, point, intensity=1.0, n=200000):
    """radiance along the ray o + t d from one isotropic scattering of a point emitter's light in a homogeneous medium occupying
    [t_enter, t_exit] of the ray (the emitter inside it):  int sigma_s e^{-sigma_t (t - t_enter)} (1/4pi) I e^{-sigma_t |x(t) - q|} / |x(t) - q|^2 dt
    (midpoint rule).  Returns (total, t, integrand * dt) so that callers can bin the contributions by path length."""
    st = sigma_a + sigma_s
    L = t_exit - t_enter
    t = t_enter + (np.arange(n) + 0.5) / n * L
    x = np.asarray(o, np.float64)[None] + t[:, None] * np.asarray(d, np.float64)[None]
    r = np.linalg.norm(np.asarray(point, np.float64)[None] - x, axis=1)
    f = sigma_s * np.exp(-st * (t - t_enter)) * INV_FOURPI * intensity * np.exp(-st * r) / (r * r) * (L / n)
    return f.sum(), t, f, r
