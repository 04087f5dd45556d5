"""Area emitters on `sphere` and `disk` shapes beside the rectangle (MER_EMITTER_AREA_DISK / MER_EMITTER_AREA_SPHERE).  The oracle does not know
these shapes: the yardsticks are tests/area_shapes64.py (the shapes' float64 restatement, pinned on closed forms by
tests/test_area_shapes64.py) for the leaf entry points, and tests/volpath64_shapes.py (an independent float64 volpath, checked by
tests/test_volpath64_shapes.py), furnaces and invariances for the renders."""
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi
from tests import area_shapes64 as A, scenes, volpath64_shapes as vs
from tests.combined_scenes import mixed_params as _mixed_params

pytestmark = pytest.mark.gpu

N_LEAF = 20000
RECT_M = np.array([[0.9, 0, 0, 0.3], [0, 0, -1, 2.0], [0, -0.6, 0, 0.1]], np.float64)             # above the cube, faces down
_c, _s = np.cos(np.deg2rad(25.0)), np.sin(np.deg2rad(25.0))
DISK_M = np.array([[0.7 * _c, 0, 0.7 * _s, -0.2], [0.7 * _s, 0, -0.7 * _c, 2.1], [0, -0.7, 0, 0.3]], np.float64)   # tilted by 25 degrees about z, scaled by 0.7, faces the cube
BALL = ([0.3, 2.4, 0.2], 0.7)
DOME = ([0.1, -0.1, 0.2], 4.0)                                                                    # inward-facing, around cube and camera
L3 = [3.0, 2.0, 1.0]


def _leaf_cases():
    return {"rectangle": (P.area_emitter(RECT_M, L3), A.Shape(A.RECT, RECT_M, L3)),
            "disk": (P.disk_emitter(DISK_M, L3), A.Shape(A.DISK, DISK_M, L3)),
            "sphere": (P.sphere_emitter(BALL[0], BALL[1], L3), A.sphere(BALL[0], BALL[1], L3)),
            "flipped_sphere": (P.sphere_emitter(DOME[0], DOME[1], L3, flip_normals=True), A.sphere(DOME[0], DOME[1], L3, flip=True))}


def _samples(name, n, seed):
    """reference points in the cube [-1, 1]^3 (inside the flipped sphere) and samples that include the concentric map's branch boundaries
    (the centre, the diagonals |r1| = |r2|, the axes) and the square's edges; the cone keeps u1 in [0, 0.999]: its edge is ill-conditioned
    in float32, and the excluded share is 0.1 % by construction"""
    r = np.random.RandomState(seed)
    ref = r.uniform(-1, 1, (n, 3)).astype(np.float32)
    u = r.uniform(0, 1, (n, 2)).astype(np.float32)
    u[0] = [0.5, 0.5]; u[1] = [0, 0]; u[2] = [0, 0.5]; u[3] = [0.5, 0]
    k = n // 20
    u[4:4 + k, 1] = u[4:4 + k, 0]                                   # r1 = r2
    u[4 + k:4 + 2 * k, 1] = np.float32(1) - u[4 + k:4 + 2 * k, 0]   # r1 = -r2
    u[4 + 2 * k:4 + 3 * k, 0] = 0.5                                 # r1 = 0
    u[4 + 3 * k:4 + 4 * k, 1] = 0.5                                 # r2 = 0
    if name == "sphere":
        u[:, 0] *= np.float32(0.999)
    return ref, u


def _scene(emitters, **kw):
    return scenes.homogeneous_scene(w=8, h=8, env_radiance=[0, 0, 0], emitters=emitters, **kw)


def _deviations(got, r64, r32, cols, label):
    """the GPU may deviate from float64 by 4 x the largest deviation of the same formulas evaluated in numpy float32 (per output column):
    operation order, fma and sincosf differ between the two float32 evaluations, the conditioning does not"""
    bad = []
    for j, c in enumerate(cols):
        cpu = float(np.max(np.abs(r32[:, j].astype(np.float64) - r64[:, j])))
        gpu = float(np.max(np.abs(got[:, j].astype(np.float64) - r64[:, j])))
        print("%s %-6s numpy float32 max |dev| %.3e   GPU max |dev| %.3e   (allowed %.3e)" % (label, c, cpu, gpu, 4 * cpu))
        if not gpu <= 4 * cpu:
            bad.append((c, cpu, gpu))
    return bad


DIRECT_COLS = ["v.r", "v.g", "v.b", "d.x", "d.y", "d.z", "dist", "pdf", "n.x", "n.y", "n.z"]


@pytest.mark.parametrize("name", ["rectangle", "disk", "sphere", "flipped_sphere"])
def test_area_direct_matches_float64(ctx, name):
    """mer_area_direct against tests/area_shapes64.sample_direct at 20 000 points; the table this test prints has every column.  Measured
    maxima of |deviation from float64|, numpy float32 | GPU (MI355X), largest value column and the pdf:
        rectangle        value 1.695e-06 | 1.696e-06    pdf 1.618e-06 | 1.858e-06    d 1.31e-07 | 1.48e-07
        disk             value 1.316e-06 | 1.555e-06    pdf 3.448e-06 | 3.448e-06    d 1.38e-07 | 1.48e-07
        sphere           value 1.255e-06 | 1.353e-06    pdf 1.765e-05 | 1.765e-05    n 1.606e-04 | 1.606e-04
        flipped sphere   value 2.014e-03 | 2.012e-03    pdf 8.979e-06 | 8.971e-06    dist 2.075e-04 | 2.075e-04   (values are ~50: L / pdf)
    The GPU never exceeded 1.3 x the numpy float32 maximum of a column; 4 x is allowed."""
    em, sh = _leaf_cases()[name]
    sc, _ = ctx.upload_scene(_scene([em]))
    ref, u = _samples(name, N_LEAF, 7)
    got = ctx.area_direct(sc, 0, ref, u)
    assert got.shape == (N_LEAF, 12) and np.all(got[:, 11] == 0)
    r64 = np.column_stack(A.sample_direct(sh, ref, u, np.float64))
    r32 = np.column_stack(A.sample_direct(sh, ref, u, np.float32))
    # sidedness and the zero / non-zero pattern agree exactly away from grazing directions (|d . n| > 1e-4)
    clear = np.abs((r64[:, 3:6] * r64[:, 8:11]).sum(1)) > 1e-4
    assert clear.mean() > 0.99
    assert np.array_equal(got[clear, 7] > 0, r64[clear, 7] > 0) and np.array_equal(got[clear, :3] > 0, r64[clear, :3] > 0)
    lit = clear & (r64[:, 7] > 0)
    assert lit.sum() > (N_LEAF // 4 if name != "flipped_sphere" else N_LEAF - 1)
    assert np.all(got[clear & ~lit, :3] == 0) and np.all(got[clear & ~lit, 7] == 0)            # the back side: exactly nothing
    bad = _deviations(got[lit], r64[lit], r32[lit], DIRECT_COLS, name)
    assert not bad, bad


def _grown(sh, f):
    """the shape with its extent scaled by f about its centre (the plane and the centre stay)"""
    m = np.eye(4); m[:3, :4] = sh.M
    m[:3, :3] *= f
    return A.Shape(sh.kind, m, sh.L)


@pytest.mark.parametrize("name", ["three_shapes", "flipped_sphere"])
def test_area_hit_matches_float64(ctx, name):
    """mer_area_hit against tests/area_shapes64: the nearest of a rectangle, a disk and an outward sphere (the disk hides part of the
    sphere, the rectangle part of the disk), or the enclosing flipped sphere from inside; pdfDirect from reference points that are not
    the rays' origins.  Index, sidedness and the zero pattern agree exactly wherever the float64 answer does not change when every shape
    grows or shrinks by 1e-4; t and the pdf by the float32 rule of test_area_direct_matches_float64.  Measured maxima, numpy float32 | GPU:
    three shapes t 2.230e-06 | 2.290e-06, pdf 3.340e-03 | 3.905e-03 (the pdf is large where a hit is grazing); flipped sphere t 4.758e-07 |
    4.758e-07, pdf 6.009e-08 | 6.925e-08."""
    cases = _leaf_cases()
    names = ["rectangle", "disk", "sphere"] if name == "three_shapes" else ["flipped_sphere"]
    sc, _ = ctx.upload_scene(_scene([P.point_emitter([0, 0, 0], [1, 1, 1])] + [cases[k][0] for k in names]))      # a point entry first: list index = slot + 1
    shapes = [cases[k][1] for k in names]
    r = np.random.RandomState(11)
    o = r.uniform(-1, 1, (N_LEAF, 3)).astype(np.float32)
    if name == "three_shapes":                                      # half of the rays start around and above the shapes (some inside the sphere): back sides
        o[N_LEAF // 2:] = (r.uniform(-1, 1, (N_LEAF - N_LEAF // 2, 3)) * [1.5, 1.4, 1.5] + [0, 2.6, 0]).astype(np.float32)
    target = np.array([0.1, 2.1, 0.2]) + r.uniform(-1.3, 1.3, (N_LEAF, 3)) * [1.0, 0.5, 1.0] if name == "three_shapes" else r.normal(size=(N_LEAF, 3)) + o
    d = (target - o); d = (d / np.linalg.norm(d, axis=1)[:, None] * r.uniform(0.5, 2.0, (N_LEAF, 1))).astype(np.float32)   # d need not be unit
    ref = (o + r.uniform(-0.3, 0.3, (N_LEAF, 3))).astype(np.float32) if name == "three_shapes" else r.uniform(-1, 1, (N_LEAF, 3)).astype(np.float32)
    got = ctx.area_hit(sc, o, d, ref)
    assert got.shape == (N_LEAF, 8) and np.all(got[:, 6:] == 0)

    def answer(shs, f):
        idx, t = A.nearest(shs, o, d, f=f)
        hit = idx >= 0
        p = o.astype(f) + d.astype(f) * t[:, None]
        Le = np.zeros((N_LEAF, 3), f); pdf = np.zeros(N_LEAF, f); cosine = np.ones(N_LEAF)
        for j, sh in enumerate(shs):
            m = idx == j
            if m.any():
                Le[m] = A.radiance(sh, p[m], d[m], f)
                dr = p[m] - ref[m].astype(f); dist = np.sqrt((dr * dr).sum(1)); dr = dr / dist[:, None]
                pdf[m] = A.pdf_direct(sh, ref[m], dr, dist, f)
                nn = A.normal_at(sh, p[m], f)
                cosine[m] = np.minimum(np.abs((nn * d[m]).sum(1)) / np.linalg.norm(d[m], axis=1), np.abs((nn * dr).sum(1)))
        return idx, t, Le, pdf, hit, cosine
    idx, t, Le, pdf, hit, cosine = answer(shapes, np.float64)
    robust = cosine > 1e-4
    for f in (1 - 1e-4, 1 + 1e-4):
        robust &= A.nearest([_grown(s, f) for s in shapes], o, d)[0] == idx
    assert robust.mean() > 0.98 and hit[robust].mean() > 0.3 and (name != "three_shapes" or all((idx[robust] == j).sum() > 500 for j in range(3)))
    assert np.array_equal(got[robust, 0], np.where(hit, idx + 1, -1)[robust].astype(np.float32))
    assert np.all(got[robust & ~hit, 1] == -1) and np.all(got[robust & ~hit, 2:6] == 0)
    rh = robust & hit
    assert np.array_equal(got[rh, 2:5], Le[rh].astype(np.float32))                              # the radiance or exactly 0 from behind
    assert np.array_equal(got[rh, 5] > 0, pdf[rh] > 0)
    assert (Le[rh, 0] > 0).sum() > 500 and (name != "three_shapes" or (Le[rh, 0] == 0).sum() > 500)
    _, t32, _, pdf32, _, _ = answer(shapes, np.float32)
    bad = _deviations(got[rh][:, [1, 5]], np.column_stack([t, pdf])[rh], np.column_stack([t32, pdf32])[rh], ["t", "pdf"], name)
    assert not bad, bad


def test_leaf_refusals(ctx):
    sc, _ = ctx.upload_scene(_scene([P.point_emitter([0, 0, 0], [1, 1, 1]), _leaf_cases()["disk"][0]]))
    z = np.zeros((1, 3), np.float32)
    with pytest.raises(capi.MerError, match="must be an area emitter"):
        ctx.area_direct(sc, 0, z, np.zeros((1, 2), np.float32))
    with pytest.raises(capi.MerError, match="point or spot"):                                   # mer_emitter_direct keeps refusing area entries
        ctx.emitter_direct(sc, 1, z)
    with pytest.raises(capi.MerError, match="out of range"):
        ctx.area_direct(sc, 2, z, np.zeros((1, 2), np.float32))
    sp, _ = ctx.upload_scene(_scene([P.point_emitter([0, 0, 0], [1, 1, 1])]))
    with pytest.raises(capi.MerError, match="no area emitter"):
        ctx.area_hit(sp, z, z + 1, z)


# ---- renders

CAM = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
NEAR_BALL = ([-2.0, 0.2, 0.3], 0.2)                              # between the camera and the cube
NEAR_DISK = np.array([[0, 0, -1, -2.0], [0, 0.3, 0, -0.25], [0.3, 0, 0, -0.4]], np.float64)       # facing the camera (-x): det > 0, normal = column 2


def _covered(ctx, sc, sh, w, h):
    """pixels whose four corners and centre all look at the (convex) shape: every ray through them does"""
    ys, xs = np.mgrid[0:h, 0:w]
    ok = np.ones((h, w), bool)
    for dx, dy in ((0, 0), (1, 0), (0, 1), (1, 1), (0.5, 0.5)):
        o, d = ctx.camera_rays(sc, np.stack([xs.ravel() + dx, ys.ravel() + dy], 1).astype(np.float32))
        ok &= (A.intersect(sh, o, d) > 0).reshape(h, w)
    return ok


def test_direct_view(ctx):
    """camera rays that meet a sphere or a disk front before the medium carry exactly its radiance; a disk seen from behind exactly 0 (and
    it hides what lies behind it).  With hide_emitters such a pixel carries what a pixel that sees the environment carries under
    hide_emitters -- volpath.cpp:195,207 hide the directly seen emitter and the directly seen environment alike, and the shape still ends
    the ray (it is an occluder whether shown or not, as the rectangle is: tests/test_oracle_kat.py test_area_emitter_direct_view)"""
    w = h = 32
    base = scenes.homogeneous_scene(w=w, h=h, env_radiance=[0.25, 0.5, 0.75], cam_to_world=CAM, fov_x_deg=60.0, rfilter=P.FILTER_BOX, rfilter_param=0.5)
    ball = A.sphere(NEAR_BALL[0], NEAR_BALL[1], L3); disk = A.Shape(A.DISK, NEAR_DISK, [1, 2, 4])
    back = NEAR_DISK.copy(); back[:, 2] *= -1                                                    # negative determinant: the normal turns away from the camera
    ems = [P.sphere_emitter(NEAR_BALL[0], NEAR_BALL[1], L3), P.disk_emitter(NEAR_DISK, [1, 2, 4], 0.5)]
    sc, _ = ctx.upload_scene(base.copy(emitters=ems))
    on_ball, on_disk = _covered(ctx, sc, ball, w, h), _covered(ctx, sc, disk, w, h)
    assert on_ball.sum() >= 4 and on_disk.sum() >= 8 and not (on_ball & on_disk).any()
    for s in range(3):
        x = ctx.render_paths(sc, s, seed=5)
        assert np.all(x[on_ball] == np.float32(L3)) and np.all(x[on_disk] == np.float32([1, 2, 4]))
    sb, _ = ctx.upload_scene(base.copy(emitters=[ems[0], P.disk_emitter(back, [1, 2, 4], 0.5)]))
    x = ctx.render_paths(sb, 0, seed=5)
    assert np.all(x[on_disk] == 0) and np.all(x[on_ball] == np.float32(L3))
    sh, _ = ctx.upload_scene(base.copy(emitters=ems, hide_emitters=True))
    x = ctx.render_paths(sh, 0, seed=5)
    sky = np.zeros((h, w), bool); sky[0, :] = True                                               # the top row looks past everything
    o, d = ctx.camera_rays(sh, np.stack([np.arange(w) + 0.5, np.full(w, 0.5)], 1).astype(np.float32))
    assert np.all(A.nearest([ball, disk], o, d)[0] < 0)
    assert np.all(x[sky] == x[0, 0]) and np.all(x[on_ball] == x[0, 0]) and np.all(x[on_disk] == x[0, 0]) and np.all(x[0, 0] == 0)


def _dome_scene(albedo, radiance, env, w=32, h=32, **kw):
    em = [P.sphere_emitter(DOME[0], DOME[1], [radiance] * 3, flip_normals=True)] if radiance else []
    return scenes.straight_scene(N=16, w=w, h=h, albedo=[albedo] * 3, phase=P.PHASE_HG, g=0.6, env_radiance=[env] * 3, emitters=em,
                                 rfilter=P.FILTER_BOX, rfilter_param=0.5, **kw)


def _paths(ctx, p, K, seed):
    sc, vols = ctx.upload_scene(p)
    x = np.stack([ctx.render_paths(sc, k, seed=seed)[..., 0] for k in range(K)]).astype(np.float64)
    for v in vols:
        v.destroy()
    return x


def test_furnace(ctx):
    """albedo 1 in a gridded sigma_t, HG g = 0.6, no environment, inside an inward-facing sphere of radiance 1: every path carries 1 in
    expectation.  32 x 32 pixels x 64 sample indices; the standard error comes from the per-path sample variance."""
    x = _paths(ctx, _dome_scene(1.0, 1.0, 0.0), 64, seed=3)
    se = np.sqrt(x.var() / x.size)
    print("furnace: mean %.6f, standard error %.6f, per-path variance %.4f" % (x.mean(), se, x.var()))
    assert x.var() > 0
    assert abs(x.mean() - 1) < 4 * se, (x.mean(), se)


def test_dome_equals_the_constant_environment(ctx):
    """albedo 0.9: the enclosing flipped sphere of radiance L lights the medium as the constant environment of radiance L does"""
    a = _paths(ctx, _dome_scene(0.9, 0.8, 0.0), 32, seed=4)
    b = _paths(ctx, _dome_scene(0.9, 0.0, 0.8), 32, seed=5)
    se = np.sqrt(a.var() / a.size + b.var() / b.size)
    print("dome %.6f, environment %.6f, 4 sigma of the difference %.6f" % (a.mean(), b.mean(), 4 * se))
    assert a.mean() > 0.5 and abs(a.mean() - b.mean()) < 4 * se, (a.mean(), b.mean(), se)


def test_render_matches_the_float64_volpath(ctx):
    """an outward sphere, a disk that hides part of it from the cube, and a rectangle, with sampling weights 1 : 0.5 : 2, every emitter
    at least 0.5 from the cube, environment 0.2: the per-pixel z-test of tests/test_gpu_multi_emitter.py against tests/volpath64_shapes.py
    (which samples EVERY emitter at every vertex, spheres uniformly by area) -- 1024 GPU paths per pixel against 4096, at most 1 + 1 % of
    the pixels beyond 4 sigma, and the image total within 4 sigma.  Measured: 1 pixel beyond 4 sigma (max |z| 5.73), totals 72.681 (GPU)
    against 72.620; two seeds of the reference against each other: 0 pixels (tests/test_volpath64_shapes.py)."""
    ref_m, ref_v = vs.mixed_reference(1)
    S, K = vs.MIXED_SPP, 1024
    x = _paths(ctx, _mixed_params(), K, seed=11)
    z = (x.mean(0) - ref_m) / np.sqrt(x.var(0) / K + ref_v / S + 1e-14)
    print("mixed scene: max |z| %.2f, %d pixels beyond 4 sigma; totals %.4f (GPU) %.4f (float64)" % (np.abs(z).max(), (np.abs(z) > 4).sum(), x.mean(0).sum(), ref_m.sum()))
    assert (np.abs(z) > 4).sum() <= 1 + 0.01 * z.size, (np.abs(z).max(), (np.abs(z) > 4).sum())
    tg, tr = x.sum((1, 2)), ref_m.sum()
    assert abs(tg.mean() - tr) < 4 * np.sqrt(tg.var() / K + ref_v.sum() / S), (tg.mean(), tr)
    assert ref_m.mean() > 0.1


def _mixed_gridded():
    p = _mixed_params()
    q = scenes.straight_scene(N=16, w=24, h=20, albedo=[0.9] * 3, phase=P.PHASE_HG, g=0.5, env_radiance=[0.2] * 3, emitters=p.emitters)
    return q


def test_inline_walks_change_no_path(ctx):
    sc, vols = ctx.upload_scene(_mixed_gridded())
    a = np.stack([ctx.render_paths(sc, s, seed=3) for s in range(2)])
    with ctx.options(inline_walks=0):
        b = np.stack([ctx.render_paths(sc, s, seed=3) for s in range(2)])
    assert a.max() > 0 and np.array_equal(a, b)
    for v in vols:
        v.destroy()


def test_transient_frames_sum_to_the_steady_film(ctx):
    p = _mixed_params(w=24, h=20, decomposition=P.DECOMPOSITION_TRANSIENT, min_bound=0.0, max_bound=64.0, bin_width=4.0)
    sc, _ = ctx.upload_scene(p)
    film = ctx.render_to_host(sc, 0, 8, seed=5)
    ss, _ = ctx.upload_scene(p.copy(decomposition=P.DECOMPOSITION_NONE))
    steady = ctx.render_to_host(ss, 0, 8, seed=5)
    assert steady[..., :3].sum() > 0
    np.testing.assert_allclose(film[..., :-2].reshape(p.height, p.width, 16, 3).sum(2), steady[..., :3], rtol=1e-4, atol=1e-5)


def test_multi_context_matches_the_single_context(ctx):
    p = _mixed_gridded()
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


def test_check_build_renders_the_shapes_in_bounds():
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for p in (_mixed_gridded(), _dome_scene(0.9, 1.0, 0.0, w=16, h=16)):
            sc, vols = c.upload_scene(p)
            f = c.render_to_host(sc, 0, 2, seed=1)
            assert np.isfinite(f).all() and f[..., :3].sum() > 0
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (kind, idx, lim)
            for v in vols:
                v.destroy()
    finally:
        c.close()


def _rows(m):
    return [float(v) for v in np.asarray(m, np.float32)[:3, :4].reshape(-1)]


def test_render_refusals(ctx):
    """mer_render's own checks (capi's validation is bypassed by writing the entry after it)"""
    ball = P.sphere_emitter(BALL[0], BALL[1], [1, 1, 1]); disk = P.disk_emitter(DISK_M, [1, 1, 1])

    def refused(p, match, entry=0, to_world=None, then=None):
        sc, vols = ctx.upload_scene(p)
        if to_world is not None:
            sc._emitters_keep[entry].to_world[:] = _rows(to_world)
        if then:
            then(sc)
        with pytest.raises(capi.MerError, match=match):
            ctx.render_to_host(sc, 0, 1)
        for v in vols:
            v.destroy()
    ok = _scene([ball, disk])
    sc, _ = ctx.upload_scene(ok)
    ctx.render_to_host(sc, 0, 1)
    # curved rays / a dielectric boundary: the entry's type is written after capi has accepted a point emitter in its place
    curved = scenes.curved_scene(N=16, w=8, h=8, emitters=[P.point_emitter([0, 0.1, 0], [1, 1, 1])])

    def as_sphere(sc):
        sc._emitters_keep[0].type = P.EMITTER_AREA_SPHERE; sc._emitters_keep[0].to_world[:] = _rows(ball["to_world"]); sc._emitters_keep[0].radiance[:] = [1, 1, 1]
    refused(curved, "straight rays", then=as_sphere)
    refused(scenes.homogeneous_scene(w=8, h=8, boundary_bsdf=P.BSDF_HDIELECTRIC, emitters=[P.point_emitter([0, 0.1, 0], [1, 1, 1])]), "index-matched", then=as_sphere)
    refused(ok, "sphere must be clear", 0, P.sphere_emitter([0, 1.5, 0], 0.7, [1, 1, 1])["to_world"])                       # meets the cube
    refused(ok, "sphere must be clear", 0, P.sphere_emitter([1.0, 0, 0], 1.5, [1, 1, 1], flip_normals=True)["to_world"])     # flipped, cuts the cube
    sheared = np.array(DISK_M); sheared[:, 1] += 0.3 * sheared[:, 0]
    refused(ok, "contains shear", 1, sheared)
    squashed = np.array(ball["to_world"]); squashed[1, 1] = 0.5
    refused(ok, "non-uniform scale", 0, squashed)
    with_point = _scene([disk, P.point_emitter([0, 0.2, 0], [1, 1, 1])])

    def move_out(sc):
        sc._emitters_keep[1].position[:] = [0, 3, 0]
    refused(with_point, "cannot be combined with an area emitter", then=move_out)
