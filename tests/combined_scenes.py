"""The scenes that exercise the features of the EXTRA / AREA kernels together, shared by the tests that render them: the three scenes of
tests/test_gpu_combined.py (a lens or parallel sensor, an emitter list that mixes points, spots and rectangles with unequal sampling
weights, an environment map) and the mixed-shapes scene of tests/test_gpu_area_shapes.py.  Each builder returns the GPU's SceneParams next to
what the float64 volpaths take.  No GPU needed."""
import numpy as np
from mitsubaer_amd import params as P
from tests import scenes, sensors64 as S, volpath64_multi as vm, volpath64_shapes as vs, volpath64_spot as vsp
from tests.envmap64 import EnvMap64, rot


def scaled(cam, s):
    m = np.asarray(cam, np.float64).copy()
    m[:3, :3] = m[:3, :3] * np.asarray(s, np.float64)[None, :]
    return m.astype(np.float32)


CAM = P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])
WIDE = scaled(CAM, (1.3, 1.3, 1.0))
MEDIUM = dict(sigma_mode=P.SIGMA_HOMOGENEOUS, sigma_s=[1.0] * 3, sigma_a=[0.5] * 3, phase=P.PHASE_HG, g=0.5, max_depth=-1, rfilter=P.FILTER_BOX, rfilter_param=0.5)
MED64 = (1.0, 0.5, 0.5)
ROT = rot([0.3, 1.0, -0.4], 57.0)


def sun_map():
    """a 16 x 8 lat-long map: dim everywhere, one bright 2 x 2 'sun'"""
    img = np.full((8, 16, 3), 0.05, np.float32)
    img[2:4, 9:11] = [40.0, 30.0, 20.0]
    return img


def sun_direction(to_world):
    """the world direction of the sun's centre (texel corner (10, 3) of the 16 x 8 map)"""
    phi, theta = 2 * np.pi * 10 / 16, np.pi * 3 / 8
    d = np.array([np.sin(phi) * np.sin(theta), np.cos(theta), -np.cos(phi) * np.sin(theta)])
    return np.asarray(to_world, np.float64)[:3, :3] @ d


def facing_rect(centre, half):
    """the 3 x 4 map of a square of half side `half` at `centre` whose normal points at the origin"""
    n = -np.asarray(centre, np.float64) / np.linalg.norm(centre)
    a = np.cross(n, [0.0, 0.0, 1.0]); a /= np.linalg.norm(a)
    b = np.cross(n, a)
    m = np.stack([half * a, half * b, np.cross(a, b), np.asarray(centre, np.float64)], 1)
    assert np.dot(m[:, 2], n) > 0.999
    return m


def frame(position, target):
    """a spot's toWorld: at position, its axis towards target"""
    return np.asarray(P.look_at(position, target, [0.2, 1.0, 0.1]), np.float64)


SHADE = facing_rect(2.1 * sun_direction(ROT), 0.7)                               # between the sun and the cube
RECT_ABOVE = np.array([[1.5, 0, 0, 0], [0, 0, -1, 2.5], [0, -1.5, 0, 0]], np.float64)
RECT_NEAR = np.array([[0.6, 0, 0, 0.8], [0, 0, -1, 1.6], [0, -0.6, 0, 0]], np.float64)    # under RECT_ABOVE: hides part of it
SPOT_AT = [0.5, 0.4, -0.3]
NAMES = ["lens_map_spot_point_rect", "lens_two_rects_two_spots", "parallel_map_points"]


def scene(name):
    """-> (SceneParams of the GPU render, arguments of volpath64_all.render, the same with the scene's interaction removed)"""
    if name == "lens_map_spot_point_rect":
        sensor = dict(sensor=P.SENSOR_THINLENS, cam_to_world=CAM, aperture_radius=0.3, focus_distance=3.0)
        across = frame([0.6, -0.5, 0.4], [-0.6, 0.5, -0.3])
        ems = [P.envmap_emitter(sun_map(), ROT), P.spot_emitter(across, [2.0] * 3, 60.0, weight=3.0), P.point_emitter([-0.3, 0.3, 0.5], [1.0] * 3, 1.0),
               P.area_emitter(SHADE, [0.5] * 3, 2.0)]
        ref = dict(kind=S.THINLENS, points=[([-0.3, 0.3, 0.5], 1.0)], spots=[vsp.Spot(across, 2.0, 60.0)], rects=[vm.Rect(SHADE, 0.5)], env=EnvMap64(sun_map(), ROT),
                   cam_to_world=CAM, aperture_radius=0.3, focus_distance=3.0)
        wrong = dict(ref, env_sample_sees_rects=False)
        env = [0.0] * 3
    elif name == "lens_two_rects_two_spots":
        sensor = dict(sensor=P.SENSOR_TELECENTRIC, cam_to_world=WIDE, aperture_radius=0.3, focus_distance=3.0)
        wide, narrow = frame(SPOT_AT, [0.5, -1.0, -0.3]), frame(SPOT_AT, [-0.8, -0.2, 0.4])
        ems = [P.spot_emitter(wide, [0.5] * 3, 180.0, 180.0, weight=1.0), P.spot_emitter(narrow, [12.0] * 3, 20.0, weight=2.5),
               P.area_emitter(RECT_ABOVE, [3.0] * 3, 1.0), P.area_emitter(RECT_NEAR, [1.5] * 3, 0.5)]
        ref = dict(kind=S.TELECENTRIC, points=[], spots=[vsp.Spot(wide, 0.5, 180.0, 180.0), vsp.Spot(narrow, 12.0, 20.0)],
                   rects=[vm.Rect(RECT_ABOVE, 3.0), vm.Rect(RECT_NEAR, 1.5)], env=0.2, cam_to_world=WIDE, aperture_radius=0.3, focus_distance=3.0)
        wrong = dict(ref, spots=ref["spots"][:1])
        env = [0.2] * 3
    else:
        sensor = dict(sensor=P.SENSOR_ORTHOGRAPHIC, cam_to_world=WIDE)
        pts = [([-1.6, 1.4, 0.4], 2.0), ([0.5, -1.8, 0.6], 1.0)]
        ems = [P.point_emitter(pts[0][0], [pts[0][1]] * 3, 0.5), P.envmap_emitter(sun_map(), ROT), P.point_emitter(pts[1][0], [pts[1][1]] * 3, 2.0)]
        ref = dict(kind=S.ORTHOGRAPHIC, points=pts, spots=[], rects=[], env=EnvMap64(sun_map(), ROT), cam_to_world=WIDE)
        wrong = dict(ref, env=EnvMap64(sun_map()))
        env = [0.0] * 3
    p = scenes.homogeneous_scene(w=16, h=16, fov_x_deg=50.0, env_radiance=env, emitters=ems, **MEDIUM, **sensor)
    return p, ref, wrong


def mixed_params(**kw):
    """the GPU scene of volpath64_shapes.mixed_shapes(): an outward sphere, a disk and a rectangle with sampling weights 1 : 0.5 : 2"""
    c, r, l, ws = vs.MIXED_SPHERE
    ems = [P.sphere_emitter(c, r, [l] * 3, ws), P.disk_emitter(vs.MIXED_DISK[0], [vs.MIXED_DISK[1]] * 3, vs.MIXED_DISK[2]),
           P.area_emitter(vs.MIXED_RECT[0], [vs.MIXED_RECT[1]] * 3, vs.MIXED_RECT[2])]
    m = vs.MIXED
    base = dict(w=m["width"], h=m["height"], sigma_s=[m["sigma_s"]] * 3, sigma_a=[m["sigma_a"]] * 3, phase=P.PHASE_HG, g=m["g"], env_radiance=[m["env"]] * 3,
                fov_x_deg=m["fov_x_deg"], cam_to_world=P.look_at(*vs.MIXED_CAM), rfilter=P.FILTER_BOX, rfilter_param=0.5, max_depth=-1, emitters=ems)
    base.update(kw)
    return scenes.homogeneous_scene(**base)
