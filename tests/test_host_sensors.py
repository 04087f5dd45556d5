"""The sensors beside the pinhole without a GPU: the XML vocabulary of `orthographic`, `thinlens` and `telecentric` (src/sensors/), the
sensor fields of mer_scene_desc, and the refusals of the host parser and of capi's validation."""
import numpy as np
import pytest
from mitsubaer_amd import host, params as P, capi

MED = '<medium type="homogeneous" id="m"><spectrum name="sigmaS" value="1"/><spectrum name="sigmaA" value="0.1"/></medium>'
FILM = '<film type="hdrfilm"><integer name="width" value="12"/><integer name="height" value="8"/></film>'
LOOKAT = '<lookat origin="-3, 0.2, 0.1" target="-2, 0.1, 0.3" up="0, 1, 0"/>'


def _scene(tmp_path, kind, props="", transform=LOOKAT):
    f = str(tmp_path / "s.xml")
    sensor = '<sensor type="%s"><transform name="toWorld">%s</transform>%s%s</sensor>' % (kind, transform, props, FILM)
    open(f, "w").write('<scene version="0.5.0"><integrator type="volpath"/>' + sensor + MED +
                       '<shape type="cube"><ref name="interior" id="m"/></shape></scene>')
    return f


def _f(name, v):
    return '<float name="%s" value="%g"/>' % (name, v)


def test_perspective_descriptor_has_the_new_fields_zero(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, "perspective", _f("fov", 40)))
    assert d.sensor == P.SENSOR_PERSPECTIVE == 0 and d.aperture_radius == 0.0 and d.focus_distance == 0.0 and d.sensor_reserved == 0
    assert d.fov_x_deg == 40.0
    # a `focusDistance` on a pinhole is read and has no effect, as before
    d, _ = host.flatten_xml(_scene(tmp_path, "perspective", _f("focusDistance", 3)))
    assert d.sensor == 0 and d.focus_distance == 0.0


def test_orthographic_defaults(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, "orthographic"))
    assert d.sensor == P.SENSOR_ORTHOGRAPHIC == 1
    assert d.near_clip == np.float32(1e-2) and d.far_clip == np.float32(1e4)
    assert d.aperture_radius == 0.0 and d.focus_distance == 0.0                 # no lens: the fields stay zero
    m = np.array(list(d.cam_to_world)).reshape(3, 4)
    assert np.allclose(m, np.asarray(P.look_at([-3, 0.2, 0.1], [-2, 0.1, 0.3], [0, 1, 0]))[:3], atol=1e-6)


def test_thinlens_parameters_and_the_focus_default(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, "thinlens", _f("apertureRadius", 0.3) + _f("focusDistance", 3) + _f("fov", 50)))
    assert d.sensor == P.SENSOR_THINLENS == 2 and d.aperture_radius == np.float32(0.3) and d.focus_distance == 3.0 and d.fov_x_deg == 50.0
    d, _ = host.flatten_xml(_scene(tmp_path, "thinlens", _f("apertureRadius", 0.3) + _f("farClip", 250)))
    assert d.focus_distance == 250.0 and d.far_clip == 250.0                    # focusDistance defaults to farClip (sensor.cpp:162)
    d, _ = host.flatten_xml(_scene(tmp_path, "thinlens", _f("apertureRadius", 0.3)))
    assert d.focus_distance == np.float32(1e4)
    # fovAxis is read by the perspective kinds: 12 x 8, fov 40 on y
    d, _ = host.flatten_xml(_scene(tmp_path, "thinlens", _f("apertureRadius", 0.3) + _f("fov", 40) + '<string name="fovAxis" value="y"/>'))
    assert np.isclose(d.fov_x_deg, np.degrees(2 * np.arctan(np.tan(np.radians(20)) * 1.5)), rtol=1e-6)


def test_thinlens_needs_a_radius_and_zero_becomes_epsilon(tmp_path):
    with pytest.raises(host.HostError, match="apertureRadius"):
        host.flatten_xml(_scene(tmp_path, "thinlens", _f("focusDistance", 3)))
    d, _ = host.flatten_xml(_scene(tmp_path, "thinlens", _f("apertureRadius", 0) + _f("focusDistance", 3)))
    assert d.aperture_radius == np.float32(1e-4)                                # Epsilon (thinlens.cpp:134-137)


def test_telecentric_defaults_and_parameters(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, "telecentric"))
    assert d.sensor == P.SENSOR_TELECENTRIC == 3 and d.aperture_radius == 0.0 and d.focus_distance == np.float32(1e4)
    d, _ = host.flatten_xml(_scene(tmp_path, "telecentric", _f("apertureRadius", 0.25) + _f("focusDistance", 2.5) + _f("nearClip", 0.5) + _f("farClip", 20)))
    assert d.aperture_radius == 0.25 and d.focus_distance == 2.5 and d.near_clip == 0.5 and d.far_clip == 20.0


@pytest.mark.parametrize("kind", ["orthographic", "telecentric"])
def test_parallel_kinds_take_a_scaled_to_world(tmp_path, kind):
    tr = '<scale x="1.5" y="0.75" z="2"/>' + LOOKAT
    d, _ = host.flatten_xml(_scene(tmp_path, kind, "", tr))
    m = np.array(list(d.cam_to_world)).reshape(3, 4)
    look = np.asarray(P.look_at([-3, 0.2, 0.1], [-2, 0.1, 0.3], [0, 1, 0]), np.float64)[:3]
    assert np.allclose(np.linalg.norm(m[:, :3], axis=0), [1.5, 0.75, 2.0], rtol=1e-6)          # the extent of the view is the scale
    assert np.allclose(m[:, :3], look[:, :3] * [1.5, 0.75, 2.0], atol=1e-6) and np.allclose(m[:, 3], look[:, 3], atol=1e-6)


@pytest.mark.parametrize("kind, props, transform, match", [
    ("orthographic", "", '<scale x="1" y="0" z="1"/>', "singular"),
    ("telecentric", _f("apertureRadius", -0.1), LOOKAT, "apertureRadius"),
    ("thinlens", _f("apertureRadius", -0.1), LOOKAT, "apertureRadius"),
    ("thinlens", _f("apertureRadius", 0.1) + _f("focusDistance", 0), LOOKAT, "focusDistance"),
    ("telecentric", _f("focusDistance", -2), LOOKAT, "focusDistance"),
    ("orthographic", _f("nearClip", 0), LOOKAT, "nearClip"),
    ("orthographic", _f("nearClip", 5) + _f("farClip", 2), LOOKAT, "nearClip"),
])
def test_refused_parameters(tmp_path, kind, props, transform, match):
    with pytest.raises(host.HostError, match=match):
        host.flatten_xml(_scene(tmp_path, kind, props, transform))


@pytest.mark.parametrize("kind", ["spherical", "radiancemeter", "irradiancemeter", "fluencemeter", "perspective_rdist"])
def test_other_sensors_stay_refused_by_name(tmp_path, kind):
    with pytest.raises(host.HostError, match='sensor "%s" is not supported' % kind):
        host.flatten_xml(_scene(tmp_path, kind))


def test_params_defaults_and_capi_validation():
    p = P.SceneParams()
    assert p.sensor == P.SENSOR_PERSPECTIVE and p.aperture_radius == 0.0 and p.focus_distance == 0.0
    assert (P.SENSOR_PERSPECTIVE, P.SENSOR_ORTHOGRAPHIC, P.SENSOR_THINLENS, P.SENSOR_TELECENTRIC) == (0, 1, 2, 3)
    capi.validate_sensor(p)
    capi.validate_sensor(p.copy(sensor=P.SENSOR_ORTHOGRAPHIC))
    capi.validate_sensor(p.copy(sensor=P.SENSOR_TELECENTRIC, focus_distance=2.0))
    m = np.asarray(p.cam_to_world, np.float64).copy(); m[:3, 1] = 0
    for q, match in [(p.copy(sensor=7), "unknown sensor"), (p.copy(sensor=P.SENSOR_ORTHOGRAPHIC, cam_to_world=m), "singular"),
                     (p.copy(sensor=P.SENSOR_THINLENS, aperture_radius=-1.0, focus_distance=2.0), "aperture_radius"),
                     (p.copy(sensor=P.SENSOR_THINLENS, aperture_radius=0.1, focus_distance=0.0), "focus_distance"),
                     (p.copy(sensor=P.SENSOR_TELECENTRIC, aperture_radius=float("nan"), focus_distance=1.0), "aperture_radius")]:
        with pytest.raises(capi.MerError, match=match):
            capi.validate_sensor(q)


def test_descriptor_mirror_has_the_sensor_fields_before_the_rough_fields():
    names = [f[0] for f in capi.SceneDesc._fields_]
    i = names.index("n_emitters")
    assert names[i + 1:i + 5] == ["sensor", "aperture_radius", "focus_distance", "sensor_reserved"]
    assert names[-3:] == ["rough_distribution", "rough_alpha", "rough_sample_visible"]
    assert capi.SceneDesc.sensor.offset == capi.SceneDesc.n_emitters.offset + 4                      # no padding
    assert capi.SceneDesc.rough_distribution.offset == capi.SceneDesc.sensor.offset + 16
    assert np.all(np.frombuffer(bytes(capi.SceneDesc()), np.uint8) == 0)                             # all zero = the pinhole


def test_the_example_scene_parses():
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    d, spp = host.flatten_xml(os.path.join(root, "scenes", "cfg_thinlens.xml"), {"samples": "4"})
    assert spp == 4 and d.sensor == P.SENSOR_THINLENS and d.aperture_radius == np.float32(0.15) and d.focus_distance == 4.0 and d.fov_x_deg == 50.0
    assert list(d.area_radiance) == [6.0, 5.0, 4.0] and list(d.point_intensity) == [3.0, 3.0, 3.0]
