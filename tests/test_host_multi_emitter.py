"""Several point and area emitters without a GPU: the XML vocabulary (several `point` emitters, several `rectangle` shapes carrying `area`,
`samplingWeight`), the emitter list of mer_scene_desc, and the refusals of the host parser and of capi's validation."""
import ctypes
import os
import numpy as np
import pytest
from mitsubaer_amd import host, params as P, capi
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = '<sensor type="perspective"><film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/></film></sensor>'
MED = '<medium type="homogeneous" id="m"><spectrum name="sigmaS" value="1"/><spectrum name="sigmaA" value="0.1"/></medium>'


def _point(x, y, z, intensity="5", weight=None):
    w = '' if weight is None else '<float name="samplingWeight" value="%g"/>' % weight
    return '<emitter type="point"><point name="position" x="%g" y="%g" z="%g"/><spectrum name="intensity" value="%s"/>%s</emitter>' % (x, y, z, intensity, w)


def _rect(ty, angle, radiance="3, 2, 1", weight=None, scale=1.5):
    w = '' if weight is None else '<float name="samplingWeight" value="%g"/>' % weight
    return ('<shape type="rectangle"><transform name="toWorld"><scale x="%g" y="%g"/><rotate x="1" y="0" z="0" angle="%g"/><translate x="0" y="%g" z="0"/>'
            '</transform><emitter type="area"><spectrum name="radiance" value="%s"/>%s</emitter></shape>' % (scale, scale, angle, ty, radiance, w))


def _scene(tmp_path, extra, shape='<shape type="cube"><ref name="interior" id="m"/></shape>', med=MED):
    f = str(tmp_path / "s.xml")
    open(f, "w").write('<scene version="0.5.0"><integrator type="volpath"/>' + CAM + med + shape + extra + '</scene>')
    return f


def _entries(d):
    return [d.emitters[i] for i in range(d.n_emitters)]


def test_two_points_two_rectangles_give_the_list(tmp_path):
    extra = (_rect(2.5, 90) + _rect(-2.5, -90, "1, 2, 4", weight=0.5) +
             _point(0.2, 0.3, -0.1, "1, 0.8, 0.5") + _point(-0.4, -0.5, 0.3, "0.5, 0.5, 1", weight=3))
    d, _ = host.flatten_xml(_scene(tmp_path, extra))
    assert d.n_emitters == 4
    assert list(d.point_intensity) == [0, 0, 0] and list(d.area_radiance) == [0, 0, 0]        # the single-emitter fields stay zero
    e = _entries(d)
    assert [x.type for x in e] == [P.EMITTER_AREA, P.EMITTER_AREA, P.EMITTER_POINT, P.EMITTER_POINT]
    assert np.allclose(list(e[0].radiance), [3, 2, 1]) and e[0].sampling_weight == 1.0
    assert np.allclose(list(e[1].radiance), [1, 2, 4]) and e[1].sampling_weight == 0.5
    m0 = np.array(list(e[0].to_world)).reshape(3, 4); m1 = np.array(list(e[1].to_world)).reshape(3, 4)
    assert np.allclose(m0[:, 3], [0, 2.5, 0]) and np.allclose(m0[:, 2], [0, -1, 0], atol=1e-6)      # faces down, towards the cube
    assert np.allclose(m1[:, 3], [0, -2.5, 0]) and np.allclose(m1[:, 2], [0, 1, 0], atol=1e-6)      # faces up
    assert np.allclose(list(e[2].position), [0.2, 0.3, -0.1]) and np.allclose(list(e[2].intensity), [1, 0.8, 0.5]) and e[2].sampling_weight == 1.0
    assert np.allclose(list(e[3].position), [-0.4, -0.5, 0.3]) and e[3].sampling_weight == 3.0


def test_one_emitter_of_each_kind_keeps_the_single_fields(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, _rect(2.5, 90) + _point(0.2, 0.3, -0.1, weight=2)))
    assert d.n_emitters == 0 and not d.emitters
    assert np.allclose(list(d.area_radiance), [3, 2, 1]) and np.allclose(list(d.point_position), [0.2, 0.3, -0.1])


def test_two_points_without_rectangles(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, _point(0.2, 0.3, -0.1) + _point(0, 3, 0)))        # one inside, one outside the cube: allowed
    assert d.n_emitters == 2 and [x.type for x in _entries(d)] == [P.EMITTER_POINT] * 2


def test_host_refusals(tmp_path):
    with pytest.raises(host.HostError, match="At most 32"):
        host.flatten_xml(_scene(tmp_path, "".join(_point(0.01 * i, 0, 0) for i in range(33))))
    with pytest.raises(host.HostError, match="samplingWeight must be positive"):
        host.flatten_xml(_scene(tmp_path, _point(0, 0, 0) + _point(0.1, 0, 0, weight=0)))
    with pytest.raises(host.HostError, match="cannot be combined with an area emitter"):
        host.flatten_xml(_scene(tmp_path, _rect(2.5, 90) + _rect(-2.5, -90) + _point(0, 3, 0)))
    curved = ('<medium type="heterogeneousrefractive" id="m"><spectrum name="sigmaS" value="1"/><float name="stepsize" value="0.01"/>'
              '<volume name="rif" type="acousticrifvolume"><float name="freq" value="3000"/><float name="speed" value="1500"/>'
              '<float name="n_o" value="1.33"/><float name="n_max" value="0.05"/><integer name="mode" value="1"/></volume></medium>')
    with pytest.raises(host.HostError, match="straight rays"):
        host.flatten_xml(_scene(tmp_path, _rect(2.5, 90) + _rect(-2.5, -90), med=curved))


def test_example_scene_parses():
    d, spp = host.flatten_xml(os.path.join(ROOT, "scenes", "cfg_multi_emitter.xml"), {"samples": "4"})
    assert spp == 4 and d.n_emitters == 4
    e = _entries(d)
    assert sorted(x.type for x in e) == [P.EMITTER_POINT] * 2 + [P.EMITTER_AREA] * 2
    assert sorted(x.sampling_weight for x in e) == [0.5, 1.0, 1.0, 3.0]
    assert np.allclose(list(d.env_radiance), [0.2] * 3)
    p = scenes.homogeneous_scene(w=8, h=8, env_radiance=[0.2] * 3, emitters=[_as_param(x) for x in e])
    capi.validate_emitters(p)                                   # the same list passes capi's checks


def _as_param(x):
    if x.type == P.EMITTER_POINT:
        return P.point_emitter(list(x.position), list(x.intensity), x.sampling_weight)
    return P.area_emitter(np.array(list(x.to_world)).reshape(3, 4), list(x.radiance), x.sampling_weight)


def _rect_param(center, u, v, radiance=(1, 1, 1)):
    n = np.cross(u, v); n = n / np.linalg.norm(n)
    return P.area_emitter(np.column_stack([u, v, n, center]), radiance)


@pytest.mark.parametrize("boundary", [P.BOUNDARY_AABB, P.BOUNDARY_SPHERE])
def test_capi_refusals(boundary):
    base = scenes.homogeneous_scene(w=8, h=8, boundary=boundary)
    ok = _rect_param([0, 2.5, 0], [1.5, 0, 0], [0, 0, 1.5])
    capi.validate_emitters(base.copy(emitters=[ok, _rect_param([0, -2.5, 0], [1, 0, 0], [0, 0, 1])]))
    with pytest.raises(capi.MerError, match="at most 32"):
        capi.validate_emitters(base.copy(emitters=[P.point_emitter([0, 0, 0], [1, 1, 1])] * 33))
    with pytest.raises(capi.MerError, match="must be zero"):
        capi.validate_emitters(base.copy(emitters=[ok], point_intensity=[1, 1, 1]))
    with pytest.raises(capi.MerError, match="must be zero"):
        capi.validate_emitters(base.copy(emitters=[ok], area_radiance=[1, 1, 1]))
    # a large rectangle that cuts the shape off-centre: its four corners and its centre all lie outside (the single-rectangle test's probes)
    cut = _rect_param([3.5, 0.8, 0], [3.0, 0, 0], [0, 0, 3.0])
    corners = [np.array([3.5, 0.8, 0]) + a * np.array([3.0, 0, 0]) + b * np.array([0, 0, 3.0]) for a in (-1, 0, 1) for b in (-1, 0, 1) if a * b != 0 or a == b == 0]
    for q in corners:
        assert not capi._point_in_shape(base, q)
    with pytest.raises(capi.MerError, match="must lie outside"):
        capi.validate_emitters(base.copy(emitters=[cut]))
    # tilted: a rectangle through the middle of the shape whose probes miss it
    tilt = _rect_param([0, 0, 0], [2.5, 2.5, 0], [0, 0, 2.5])
    with pytest.raises(capi.MerError, match="must lie outside"):
        capi.validate_emitters(base.copy(emitters=[tilt]))
    with pytest.raises(capi.MerError, match="straight rays"):
        capi.validate_emitters(base.copy(emitters=[ok], rif_mode=P.RIF_TRILINEAR))
    with pytest.raises(capi.MerError, match="cannot be combined"):
        capi.validate_emitters(base.copy(emitters=[ok, P.point_emitter([0, 3, 0], [1, 1, 1])]))
    capi.validate_emitters(base.copy(emitters=[ok, P.point_emitter([0, 0.2, 0], [1, 1, 1])]))       # inside the shape: allowed
    with pytest.raises(capi.MerError, match="samplingWeight"):
        capi.validate_emitters(base.copy(emitters=[P.point_emitter([0, 0, 0], [1, 1, 1], 0.0)]))


def test_scene_desc_carries_the_list():
    p = scenes.homogeneous_scene(w=8, h=8, emitters=[P.point_emitter([0, 0.1, 0], [1, 2, 3], 2.0), P.point_emitter([0.1, 0, 0], [4, 5, 6])])

    class _NoGpu(capi.Context):
        def __init__(self):
            pass
    s = _NoGpu().scene_desc(p)
    assert s.n_emitters == 2 and s.emitters[0].type == P.EMITTER_POINT and s.emitters[0].sampling_weight == 2.0
    assert list(s.emitters[1].intensity) == [4, 5, 6]
    assert ctypes.sizeof(capi.EmitterDesc) == 4 * (1 + 3 + 3 + 12 + 3 + 1)
