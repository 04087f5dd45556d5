"""The orthographic, thin-lens and telecentric sensors on the GPU (mer_scene_desc.sensor): the leaf entry point mer_sensor_rays against
tests/sensors64.py, the sampler-stream rule (the two lens kinds draw an aperture sample after the pixel sample), known answers only a parallel
sensor has, per-pixel agreement with tests/volpath64_sensor.py, and the equivalences the pinhole is held to, for every new kind."""
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi
from tests import scenes, sensors64 as S, volpath64_multi as vm, volpath64_sensor as vs

pytestmark = pytest.mark.gpu

NEW_KINDS = [P.SENSOR_ORTHOGRAPHIC, P.SENSOR_THINLENS, P.SENSOR_TELECENTRIC]
NAMES = {P.SENSOR_PERSPECTIVE: "perspective", P.SENSOR_ORTHOGRAPHIC: "orthographic", P.SENSOR_THINLENS: "thinlens", P.SENSOR_TELECENTRIC: "telecentric"}
CAM = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])


def _scaled(cam, s):
    m = np.asarray(cam, np.float64).copy()
    m[:3, :3] = m[:3, :3] * np.asarray(s, np.float64)[None, :]
    return m.astype(np.float32)


def _sensor(kind, extent=1.3):
    """the sensor fields of the render tests: the parallel kinds see [-extent, extent]^2 around the cube; aperture 0.3 focused on the cube's centre"""
    kw = dict(sensor=kind, cam_to_world=CAM if kind in (P.SENSOR_PERSPECTIVE, P.SENSOR_THINLENS) else _scaled(CAM, (extent, extent, 1.0)), fov_x_deg=50.0)
    if kind in (P.SENSOR_THINLENS, P.SENSOR_TELECENTRIC):
        kw.update(aperture_radius=0.3, focus_distance=3.0)
    return kw


# ---- 1. the leaf: mer_sensor_rays against tests/sensors64.py

@pytest.mark.parametrize("kind", [P.SENSOR_PERSPECTIVE] + NEW_KINDS)
def test_sensor_rays_match_float64(ctx, kind):
    """every pixel corner and centre x a grid of aperture samples with the disk map's branch boundaries (u1 = u2, u1 = 1 - u2, an axis at
    0.5) and (0.5, 0.5); a rotated, translated toWorld, scaled for the parallel kinds.  1e-6 absolute on o and d (check_camera's bound for
    the pinhole) times the largest |toWorld| entry, 1e-6 relative on mint / maxt."""
    w, h, fov, near, far, radius, focus = 12, 8, 40.0, 0.0625, 64.0, 0.25, 2.75
    parallel = kind in (P.SENSOR_ORTHOGRAPHIC, P.SENSOR_TELECENTRIC)
    c2w = P.look_at([-3, 0.2, 0.1], [-2, 0.1, 0.3], [0, 1, 0])
    if parallel:
        c2w = _scaled(c2w, (1.5, 0.75, 2.0))
    p = scenes.homogeneous_scene(w=w, h=h, fov_x_deg=fov, near_clip=near, far_clip=far, cam_to_world=c2w, sensor=kind,
                                 aperture_radius=radius if kind >= P.SENSOR_THINLENS else 0.0, focus_distance=focus if kind >= P.SENSOR_THINLENS else 0.0)
    xs = np.concatenate([np.arange(w + 1), np.arange(w) + 0.5]); ys = np.concatenate([np.arange(h + 1), np.arange(h) + 0.5])
    g = np.array([0.0, 0.125, 0.25, 0.5, 0.75, 0.875, 1.0 - 2.0 ** -24])
    X, Y, U, V = np.meshgrid(xs, ys, g, g)
    pos = np.stack([X.ravel(), Y.ravel()], 1).astype(np.float32); u = np.stack([U.ravel(), V.ravel()], 1).astype(np.float32)
    sc, _ = ctx.upload_scene(p)
    o, d, mint, maxt = ctx.sensor_rays(sc, pos, u)
    T = np.asarray(c2w, np.float32).astype(np.float64)
    ro, rd, rmin, rmax = S.sensor_rays(kind, T, w, h, float(np.float32(fov)), near, far, pos.astype(np.float64), u.astype(np.float64), radius, focus)
    tol = 1e-6 * max(1.0, np.abs(T[:3]).max())
    eo, ed = np.abs(o - ro).max(), np.abs(d - rd).max()
    print("kind %d: |o| %.3g |d| %.3g (bound %.3g) mint %.3g maxt %.3g" % (kind, eo, ed, tol, np.abs(mint / rmin - 1).max(), np.abs(maxt / rmax - 1).max()))
    assert eo < tol and ed < tol, (eo, ed, tol)
    assert np.abs(mint / rmin - 1).max() < 1e-6 and np.abs(maxt / rmax - 1).max() < 1e-6
    if kind == P.SENSOR_PERSPECTIVE:
        co, cd = ctx.camera_rays(sc, pos)
        assert np.array_equal(co, o) and np.array_equal(cd, d)                    # the pinhole: mer_camera_rays bit for bit
        o2, d2, _, _ = ctx.sensor_rays(sc, pos)                                   # no aperture samples needed
        assert np.array_equal(o2, o) and np.array_equal(d2, d)
    elif kind == P.SENSOR_ORTHOGRAPHIC:
        o2, d2, _, _ = ctx.sensor_rays(sc, pos)
        assert np.array_equal(o2, o) and np.array_equal(d2, d)
    else:
        with pytest.raises(capi.MerError, match="aperture samples"):
            ctx.sensor_rays(sc, pos)


def test_library_refusals(ctx):
    p = scenes.homogeneous_scene(w=8, h=8, **_sensor(P.SENSOR_TELECENTRIC))
    sc, _ = ctx.upload_scene(p)
    ctx.render_to_host(sc, 0, 1)
    for field, value, match in [("sensor", 4, "unknown sensor"), ("sensor", -1, "unknown sensor"), ("sensor_reserved", 1, "sensor_reserved"),
                                ("aperture_radius", -0.5, "aperture_radius"), ("aperture_radius", float("nan"), "aperture_radius"),
                                ("focus_distance", 0.0, "focus_distance"), ("focus_distance", float("inf"), "focus_distance")]:
        old = getattr(sc, field)
        setattr(sc, field, value)
        with pytest.raises(capi.MerError, match=match):
            ctx.render_to_host(sc, 0, 1)
        setattr(sc, field, old)
    old = list(sc.cam_to_world)
    sc.cam_to_world[:] = [1, 0, 0, -3, 0, 0, 0, 0, 0, 0, 1, 0]
    with pytest.raises(capi.MerError, match="cam_to_world is singular"):
        ctx.render_to_host(sc, 0, 1)
    sc.cam_to_world[:] = old
    ctx.render_to_host(sc, 0, 1)


# ---- statistics: per-pixel means of the red channel and the variance of those means, from B independent batches of S samples (box
#      filter of half a pixel: a pixel's value is the mean of its own paths)

BOX = dict(rfilter=P.FILTER_BOX, rfilter_param=0.5)


def _stats(c, p, B=32, spp=64, seed=7):
    sc, vols = c.upload_scene(p)
    m = []
    for b in range(B):
        f = c.render_to_host(sc, b * spp, spp, seed=seed)
        m.append(f[..., 0].astype(np.float64) / f[..., 4])
    for v in vols:
        v.destroy()
    m = np.stack(m)
    return m.mean(0), m.var(0, ddof=1) / B


def _z(a, b):
    return (a[0] - b[0]) / np.sqrt(a[1] + b[1] + 1e-14)


def _agrees(a, b):
    """the acceptance rule of the float64 comparisons: at most 1 + 1 % of the pixels beyond 4 sigma of the combined variance, and the
    image total within 4 sigma"""
    z = _z(a, b)
    total = abs(a[0].sum() - b[0].sum()) <= 4 * np.sqrt(a[1].sum() + b[1].sum())
    print("   outliers %d of %d, max |z| %.2f, total %.5f vs %.5f" % ((np.abs(z) > 4).sum(), z.size, np.abs(z).max(), a[0].sum(), b[0].sum()))
    return (np.abs(z) > 4).sum() <= 1 + 0.01 * z.size and total


MEDIUM = dict(sigma_mode=P.SIGMA_HOMOGENEOUS, sigma_s=[1.0] * 3, sigma_a=[0.5] * 3, phase=P.PHASE_HG, g=0.5, env_radiance=[0.2] * 3, max_depth=-1, **BOX)
POINT = ([0.2, 0.3, -0.1], 3.0)
RECT = np.array([[0, 0, -1, -1.5], [0, 0.15, 0, 0.4], [0.15, 0, 0, 0.1]], np.float64)     # columns: half-axes (0,0,.15), (0,.15,0), normal (-1,0,0), centre


def _lit(kind, **kw):
    ems = [P.point_emitter(POINT[0], [POINT[1]] * 3), P.area_emitter(RECT, [4.0] * 3)]
    return scenes.homogeneous_scene(w=16, h=16, emitters=ems, **MEDIUM, **_sensor(kind), **kw)


# ---- 2. the stream rule

def test_telecentric_with_radius_zero_is_the_orthographic_view_on_two_more_draws(ctx):
    po = _lit(P.SENSOR_ORTHOGRAPHIC)
    pt = po.copy(sensor=P.SENSOR_TELECENTRIC, aperture_radius=0.0, focus_distance=3.0)
    so, _ = ctx.upload_scene(po); st, _ = ctx.upload_scene(pt)
    a = np.stack([ctx.render_paths(so, k, seed=3) for k in range(4)]); b = np.stack([ctx.render_paths(st, k, seed=3) for k in range(4)])
    assert np.isfinite(a).all() and a.max() > 0
    assert not np.array_equal(a, b)                                               # the aperture sample is drawn even though it moves nothing
    # pixels whose rays miss everything have no draw after the ray: identical there, and the rays are the same rays
    pos = np.array([[0.5, 0.5], [8.3, 7.9], [15.5, 3.25]], np.float32); u = np.full((3, 2), 0.37, np.float32)
    ro = ctx.sensor_rays(so, pos); rt = ctx.sensor_rays(st, pos, u)
    for x, y in zip(ro, rt):
        assert np.array_equal(x, y)
    assert _agrees(_stats(ctx, po, seed=5), _stats(ctx, pt, seed=6))


# ---- 3. known answers only a parallel sensor has

def test_orthographic_view_of_an_absorbing_cube_has_one_chord(ctx):
    """sigma_s = 0 in [-1, 1]^3 under a constant environment E, viewed along x: every ray inside the silhouette has chord 2, so every pixel
    wholly inside has mean E exp(-2 sigma_a) -- within 4 standard deviations of its own sample variance (medium sampling divides the
    surviving paths by the failure pdf: the per-path values are not 0 / E) plus float32 rounding -- and every pixel wholly outside is E on
    every path.  The view is 4.4 wide on 16 pixels: the silhouette edges lie inside pixels 4 and 11.  Through a pinhole the chord varies
    over the image and the same assertion fails."""
    E, sa = 0.7, 1.0
    kw = dict(w=16, h=16, sigma_mode=P.SIGMA_HOMOGENEOUS, sigma_s=[0.0] * 3, sigma_a=[sa] * 3, medium_sampling_weight=0.5, phase=P.PHASE_ISOTROPIC,
              env_radiance=[E] * 3, max_depth=-1, **BOX)
    po = scenes.homogeneous_scene(sensor=P.SENSOR_ORTHOGRAPHIC, cam_to_world=_scaled(CAM, (2.2, 2.2, 1.0)), **kw)
    pp = scenes.homogeneous_scene(sensor=P.SENSOR_PERSPECTIVE, cam_to_world=CAM, fov_x_deg=90.0, **kw)       # the front face spans the same pixels
    inside = np.zeros((16, 16), bool); inside[5:11, 5:11] = True
    outside = np.ones((16, 16), bool); outside[4:12, 4:12] = False
    want = E * np.exp(-2 * sa)

    def passes(p):
        m, v = _stats(ctx, p, B=32, spp=32, seed=9)
        dev = np.abs(m - want)[inside]; lim = 4 * np.sqrt(v[inside]) + 1e-6 * want
        print("   max deviation / limit inside the silhouette: %.2f; mean %.5f, expected %.5f" % ((dev / lim).max(), m[inside].mean(), want))
        return np.all(dev <= lim), v

    ok, v = passes(po)
    assert ok
    assert v[inside].min() > 0                                                    # medium sampling is on: the paths of a pixel differ
    so, _ = ctx.upload_scene(po)
    paths = np.stack([ctx.render_paths(so, k, seed=2) for k in range(8)])
    assert np.all(paths[:, outside] == np.float32(E))
    assert not np.all((paths[:, inside] == 0) | (paths[:, inside] == np.float32(E)))
    assert not passes(pp)[0]


def test_orthographic_transient_film_has_a_flat_arrival_time(ctx):
    """an orthographic sensor facing a rectangle emitter at distance D = 4 with nothing between, camera edge counted: every pixel's energy
    lies in the single frame of D; a pinhole spreads it over the frames of D / cos(theta).  Frames of width 0.25 from 0.125: D falls in the
    middle of frame 15, the corner pixel's 4.70 in frame 18."""
    D, R = 4.0, 3.0
    cam = P.look_at([-3, 5, 0], [0, 5, 0], [0, 1, 0])                              # looks along +x past the cube (y in [4, 6])
    rect = np.array([[0, 0, -1, -3 + D], [0, R, 0, 5.0], [R, 0, 0, 0.0]], np.float64)
    kw = dict(w=16, h=16, fov_x_deg=50.0, env_radiance=[0.0] * 3, area_to_world=rect, area_radiance=[2.0, 2.0, 2.0], decomposition=P.DECOMPOSITION_TRANSIENT,
              min_bound=0.125, max_bound=8.125, bin_width=0.25, calibrated_transient=False, **BOX)
    frames = 32

    def film(p):
        sc, _ = ctx.upload_scene(p)
        f = ctx.render_to_host(sc, 0, 16, seed=4)
        assert f.shape[2] == frames * 3 + 2
        return f[..., :-2].reshape(16, 16, frames, 3)[..., 0] / f[..., -1:]

    fo = film(scenes.homogeneous_scene(sensor=P.SENSOR_ORTHOGRAPHIC, cam_to_world=cam, **kw))
    k = int((D - 0.125) / 0.25)
    assert k == 15
    assert np.allclose(fo[..., k], 2.0, rtol=1e-6) and np.all(np.delete(fo, k, axis=2) == 0)
    fp = film(scenes.homogeneous_scene(sensor=P.SENSOR_PERSPECTIVE, cam_to_world=cam, **kw))
    assert np.allclose(fp.sum(2), 2.0, rtol=1e-6)
    first = (fp > 0).argmax(2)                                                    # the first frame with energy, per pixel
    assert first[7, 7] == k and first[0, 0] >= k + 2 and first[15, 15] >= k + 2 and np.any(fp[..., k + 1:] > 0)
    assert not np.all(np.delete(fp, k, axis=2) == 0)


# ---- 4. the absolute value: GPU against tests/volpath64_sensor.py

@pytest.mark.parametrize("kind", NEW_KINDS)
def test_render_matches_the_float64_volpath(ctx, kind):
    """HG medium in the cube, the environment, a point emitter inside and a small rectangle in front of the cube, well off the focal plane
    (distance 1.5 of 3: a blur disk of radius 0.15, the rectangle's own half size).  Per pixel against tests/volpath64_sensor.py with the
    same sensor: at most 1 + 1 % outliers beyond 4 sigma, and the image total.  The same GPU film against the float64 film of the sensor
    WITHOUT the feature under test fails the rule: the pinhole for the thin lens, the orthographic view for the telecentric lens, the
    pinhole for the orthographic view (35, 24 and 121 outliers of 256 between the float64 films themselves)."""
    sen = _sensor(kind)
    ref_kw = dict(aperture_radius=sen.get("aperture_radius", 0.0), focus_distance=sen.get("focus_distance", 1.0), spp=2048)
    args = ([POINT], [vm.Rect(RECT, 4.0)], 0.2, 1.0, 0.5, 0.5, 16, 16, 50.0)
    ref = vs.render(kind, *args, np.asarray(sen["cam_to_world"], np.float64), seed=1, **ref_kw)
    other_kind = {P.SENSOR_THINLENS: P.SENSOR_PERSPECTIVE, P.SENSOR_TELECENTRIC: P.SENSOR_ORTHOGRAPHIC, P.SENSOR_ORTHOGRAPHIC: P.SENSOR_PERSPECTIVE}[kind]
    other = vs.render(other_kind, *args, np.asarray(_sensor(other_kind)["cam_to_world"], np.float64), seed=2, spp=2048)
    gpu = _stats(ctx, _lit(kind), B=32, spp=64, seed=11)
    assert ref[0].mean() > 0.1
    ok = _agrees(gpu, (ref[0], ref[1] / 2048))
    wrong = _agrees(gpu, (other[0], other[1] / 2048))
    assert ok and not wrong


# ---- 5. orthogonality with the modes: the equivalences the pinhole is held to, for every new kind

@pytest.mark.parametrize("kind", NEW_KINDS)
def test_curved_kernels_with_index_one_equal_straight_rays(ctx, kind):
    N = 16
    kw = dict(w=16, h=16, point_position=POINT[0], point_intensity=[POINT[1]] * 3, **MEDIUM, **_sensor(kind))
    ps = scenes.homogeneous_scene(**kw)
    pc = scenes.curved_scene(N=N, rif=np.ones((N, N, N), np.float32), stepper=P.STEP_RK4, **kw)
    pc.stepsize = 0.01                                                            # a short step: the curved kernels find the boundary to within a step
    assert _agrees(_stats(ctx, ps, seed=21), _stats(ctx, pc, seed=22))


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_hdielectric_boundary_of_index_one_equals_the_null_boundary(ctx, kind):
    kw = dict(w=16, h=16, point_position=POINT[0], point_intensity=[POINT[1]] * 3, rif_const=1.0, **MEDIUM, **_sensor(kind))
    assert _agrees(_stats(ctx, scenes.homogeneous_scene(**kw), seed=23), _stats(ctx, scenes.homogeneous_scene(boundary_bsdf=P.BSDF_HDIELECTRIC, **kw), seed=24))


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_signed_distance_cube_equals_the_cube(ctx, kind):
    """f = max(|x|, |y|, |z|) - 1 on a 49^3 grid over [-1.5, 1.5]^3 (nodes on the faces): piecewise linear, zero exactly on the cube, never
    larger than the Euclidean distance"""
    g = np.linspace(-1.5, 1.5, 49)
    Z, Y, X = np.meshgrid(g, g, g, indexing="ij")
    sdf = (np.maximum(np.maximum(np.abs(X), np.abs(Y)), np.abs(Z)) - 1.0).astype(np.float32)
    kw = dict(w=16, h=16, point_position=POINT[0], point_intensity=[POINT[1]] * 3, **MEDIUM, **_sensor(kind))
    pa = scenes.homogeneous_scene(**kw)
    pb = scenes.homogeneous_scene(boundary=P.BOUNDARY_SDF, sdf=sdf, sdf_aabb=([-1.5] * 3, [1.5] * 3), **kw)
    assert _agrees(_stats(ctx, pa, seed=25), _stats(ctx, pb, seed=26))


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_one_entry_list_equals_the_point_fields(ctx, kind):
    kw = dict(w=16, h=16, **MEDIUM, **_sensor(kind))
    sa, _ = ctx.upload_scene(scenes.homogeneous_scene(point_position=POINT[0], point_intensity=[POINT[1]] * 3, **kw))
    sb, _ = ctx.upload_scene(scenes.homogeneous_scene(emitters=[P.point_emitter(POINT[0], [POINT[1]] * 3, 2.5)], **kw))
    a = np.stack([ctx.render_paths(sa, k, seed=3) for k in range(2)]); b = np.stack([ctx.render_paths(sb, k, seed=3) for k in range(2)])
    assert np.isfinite(a).all() and a.max() > 0
    assert np.array_equal(a, b)


@pytest.mark.parametrize("kind", NEW_KINDS)
def test_multi_context_forwards_the_sensor(ctx, kind):
    p = _lit(kind).copy(width=40, height=30)
    sc, _ = ctx.upload_scene(p)
    ref = ctx.render_to_host(sc, 0, 6, seed=2)
    m = capi.MultiContext([0, 0])
    try:
        msc, _ = m.upload_scene(p)
        film = m.render_to_host(msc, 0, 6, seed=2)
        assert ref[..., :3].sum() > 0
        assert np.allclose(film, ref, rtol=1e-4, atol=1e-5)
    finally:
        m.close()


def test_check_build_renders_every_kind_in_bounds_and_bit_identically(ctx):
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        N = 16
        for kind in NEW_KINDS:
            curved = scenes.curved_scene(N=N, w=24, h=20, env_radiance=[0.3] * 3, point_position=POINT[0], point_intensity=[1.0] * 3, **BOX, **_sensor(kind))
            # box filter, two samples: a pixel's film value is the sum of its own two paths, whatever order the atomics land in
            for p in (_lit(kind), curved):
                sc, vols = c.upload_scene(p)
                f = c.render_to_host(sc, 0, 2, seed=1)
                en, n, kind_, idx, lim = c.debug_bounds()
                assert n == 0, (kind_, idx, lim)
                s2, v2 = ctx.upload_scene(p)
                g = ctx.render_to_host(s2, 0, 2, seed=1)
                assert np.isfinite(f).all() and f[..., :3].sum() > 0 and np.array_equal(f, g)
                for v in vols + v2:
                    v.destroy()
    finally:
        c.close()


def test_example_scene_renders_through_the_xml_host(tmp_path):
    """scenes/cfg_thinlens.xml through the stand-alone host, against the same file with a pinhole.  The rectangle (half size 0.1, radiance 6 in
    the red channel) is 2 from the camera and the focus is at 4, so its blur disk has radius 0.15 (4 - 2) / 4 = 0.075 = 5 pixels: the pinhole
    shows it on columns 64-77, rows 14-26, and the lens spreads it.  Columns 60-62 lie outside the sharp image, where tests/sensors64.py puts
    at least 10 % of the lens's rays on the rectangle (10 % at column 60, 56 % at 64): the lens film is brighter there by 0.6 or more (0.3
    asserted: 27 pixels of 16 samples).  The blur moves light, it does not make any: over a box with 10 pixels of margin the two films carry
    the same sum to within 10 % of the rectangle's own."""
    import os
    from mitsubaer_amd import host
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    xml = open(os.path.join(root, "scenes", "cfg_thinlens.xml")).read()
    lens = host.render_xml(os.path.join(root, "scenes", "cfg_thinlens.xml"), {"samples": 16}, seed=1)
    pin = str(tmp_path / "pinhole.xml")
    open(pin, "w").write(xml.replace('<sensor type="thinlens">', '<sensor type="perspective">').replace('<float name="apertureRadius" value="0.15"/>', ""))
    sharp = host.render_xml(pin, {"samples": 16}, seed=1)
    assert lens.shape == (96, 128, 5) and np.isfinite(lens).all() and lens[..., :3].sum() > 0
    a = lens[..., 0] / lens[..., 4]; b = sharp[..., 0] / sharp[..., 4]
    gain = a[16:25, 60:63].mean() - b[16:25, 60:63].mean()
    box = (slice(4, 37), slice(54, 88))
    flux = 6.0 * 14 * 13
    print("   gain beside the sharp image %.3f, box sums %.1f (lens) %.1f (pinhole), rectangle %.0f" % (gain, a[box].sum(), b[box].sum(), flux))
    assert abs(b[17:24, 67:75].mean() - 6.0) < 1e-3                               # the pinhole sees the rectangle, which ends its rays, and nothing else there
    assert gain > 0.3
    assert abs(a[box].sum() - b[box].sum()) < 0.1 * flux
