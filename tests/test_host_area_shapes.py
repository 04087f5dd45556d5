"""Area emitters on `disk` and `sphere` shapes without a GPU: the XML vocabulary, the list entries of mer_scene_desc
(MER_EMITTER_AREA_DISK = 5, MER_EMITTER_AREA_SPHERE = 6), and the refusals of the host parser and of capi's validation.  The emitter record and
the ABI version keep their size and value."""
import ctypes
import numpy as np
import pytest
from mitsubaer_amd import host, params as P, capi
from tests import scenes
from tests.test_host_multi_emitter import CAM, MED, _entries, _point, _scene

AREA = '<emitter type="area"><spectrum name="radiance" value="%s"/>%s</emitter>'


def _area(radiance="3, 2, 1", weight=None):
    return AREA % (radiance, '' if weight is None else '<float name="samplingWeight" value="%g"/>' % weight)


def _disk(transform, extra="", **kw):
    return '<shape type="disk"><transform name="toWorld">%s</transform>%s%s</shape>' % (transform, extra, _area(**kw))


def _sphere(props, **kw):
    return '<shape type="sphere">%s%s</shape>' % (props, _area(**kw))


def _m(e):
    return np.array(list(e.to_world)).reshape(3, 4)


def test_disk_emitter(tmp_path):
    xml = _disk('<scale x="0.5" y="0.5"/><rotate x="1" y="0" z="0" angle="90"/><translate x="0.2" y="2" z="0.1"/>', weight=0.5)
    d, _ = host.flatten_xml(_scene(tmp_path, xml))
    assert d.n_emitters == 1 and list(d.area_radiance) == [0, 0, 0]           # always a list entry: the area_* fields describe a rectangle
    e = _entries(d)[0]
    assert e.type == P.EMITTER_AREA_DISK == 5 and e.sampling_weight == 0.5 and np.allclose(list(e.radiance), [3, 2, 1])
    m = _m(e)
    assert np.allclose(m[:, 3], [0.2, 2, 0.1]) and np.allclose(np.linalg.norm(m[:, 0]), 0.5) and np.allclose(m[:, 2], [0, -1, 0], atol=1e-6)   # faces down
    flipped, _ = host.flatten_xml(_scene(tmp_path, _disk('<scale x="0.5" y="0.5"/><rotate x="1" y="0" z="0" angle="90"/><translate x="0.2" y="2" z="0.1"/>',
                                                         '<boolean name="flipNormals" value="true"/>')))
    f = _m(_entries(flipped)[0])
    assert np.allclose(f[:, 2], -m[:, 2]) and np.allclose(f[:, :2], m[:, :2]) and np.linalg.det(f[:, :3]) * np.linalg.det(m[:, :3]) < 0
    capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, emitters=[P.disk_emitter(m, list(e.radiance), e.sampling_weight)]))


def test_sphere_emitter_center_radius(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, _sphere('<point name="center" x="0.3" y="2.4" z="0.2"/><float name="radius" value="0.7"/>', radiance="5")))
    assert d.n_emitters == 1
    e = _entries(d)[0]
    assert e.type == P.EMITTER_AREA_SPHERE == 6 and e.sampling_weight == 1.0 and list(e.radiance) == [5, 5, 5]
    assert np.allclose(_m(e), np.column_stack([np.diag([0.7, 0.7, 0.7]), [0.3, 2.4, 0.2]]))
    assert d.boundary == P.BOUNDARY_AABB                                       # the cube stays the medium shape
    q = P.sphere_emitter([0.3, 2.4, 0.2], 0.7, [5, 5, 5])
    assert np.allclose(np.asarray(q["to_world"])[:3], _m(e)) and q["type"] == P.EMITTER_AREA_SPHERE


def test_sphere_emitter_scaling_to_world(tmp_path):
    """Sphere's constructor (sphere.cpp:113-122): the scale s = |toWorld e_x| multiplies the radius; the rotation does not matter"""
    xml = _sphere('<float name="radius" value="0.5"/><transform name="toWorld"><scale value="1.4"/><rotate x="0" y="0" z="1" angle="30"/><translate x="0" y="-3" z="0"/></transform>')
    d, _ = host.flatten_xml(_scene(tmp_path, xml))
    e = _entries(d)[0]
    assert e.type == P.EMITTER_AREA_SPHERE
    assert np.allclose(_m(e), np.column_stack([np.diag([0.7, 0.7, 0.7]), [0, -3, 0]]), atol=1e-6)


def test_sphere_emitter_flip_normals(tmp_path):
    xml = _sphere('<float name="radius" value="3"/><boolean name="flipNormals" value="true"/>')
    d, _ = host.flatten_xml(_scene(tmp_path, xml))
    m = _m(_entries(d)[0])
    assert np.linalg.det(m[:, :3]) < 0 and np.allclose(np.abs(np.diag(m[:, :3])), 3)      # a negative determinant is the flip
    q = P.sphere_emitter([0, 0, 0], 3, [1, 1, 1], flip_normals=True)
    assert np.allclose(np.asarray(q["to_world"])[:3], m)
    capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, emitters=[q]))              # around the cube: farthest corner sqrt(3) < 3


def test_mixed_list_is_in_scene_order(tmp_path):
    from tests.test_host_multi_emitter import _rect
    extra = (_sphere('<point name="center" x="0" y="3" z="0"/><float name="radius" value="0.5"/>') + _rect(-2.5, -90, weight=2) +
             _disk('<translate x="0" y="0" z="-2"/>') + _point(0.1, 0.2, 0.3))
    d, _ = host.flatten_xml(_scene(tmp_path, extra))
    assert [x.type for x in _entries(d)] == [P.EMITTER_AREA_SPHERE, P.EMITTER_AREA, P.EMITTER_AREA_DISK, P.EMITTER_POINT]


def test_host_refusals(tmp_path):
    with pytest.raises(host.HostError, match="contains shear"):
        host.flatten_xml(_scene(tmp_path, _disk('<matrix value="1 0.3 0 0  0 1 0 2  0 0 1 0  0 0 0 1"/>')))
    with pytest.raises(host.HostError, match="non-uniform scale"):
        host.flatten_xml(_scene(tmp_path, _disk('<scale x="1" y="0.5"/><translate x="0" y="0" z="-2"/>')))
    with pytest.raises(host.HostError, match="carrier of an area emitter only"):
        host.flatten_xml(_scene(tmp_path, '<shape type="disk"><transform name="toWorld"><translate x="0" y="0" z="-2"/></transform></shape>'))
    with pytest.raises(host.HostError, match="cannot also bound an 'interior' medium"):
        host.flatten_xml(_scene(tmp_path, "", shape='<shape type="sphere"><ref name="interior" id="m"/>' + _area() + '</shape>'))
    with pytest.raises(host.HostError, match="cannot be combined with an area emitter"):
        host.flatten_xml(_scene(tmp_path, _disk('<translate x="0" y="0" z="-2"/>') + _point(0, 0.1, 0) + _point(0, 3, 0)))
    with pytest.raises(host.HostError, match="straight rays"):
        curved = ('<medium type="heterogeneousrefractive" id="m"><spectrum name="sigmaS" value="1"/><float name="stepsize" value="0.01"/>'
                  '<volume name="rif" type="acousticrifvolume"><float name="freq" value="3000"/><float name="speed" value="1500"/>'
                  '<float name="n_o" value="1.33"/><float name="n_max" value="0.05"/><integer name="mode" value="1"/></volume></medium>')
        host.flatten_xml(_scene(tmp_path, _disk('<translate x="0" y="0" z="-2"/>') + _point(0, 0.1, 0) + _point(0, 0.2, 0), med=curved))
    # a rotated sphere that bounds the medium stays refused; one that carries an emitter is accepted
    rot = '<transform name="toWorld"><rotate x="0" y="0" z="1" angle="30"/><translate x="0" y="3" z="0"/></transform>'
    with pytest.raises(host.HostError, match="only scale \\+ translate"):
        host.flatten_xml(_scene(tmp_path, "", shape='<shape type="sphere">' + rot + '<ref name="interior" id="m"/></shape>'))
    host.flatten_xml(_scene(tmp_path, _sphere(rot)))


def _disk_param(center, u, v, radiance=(1, 1, 1), flip=False):
    n = np.cross(u, v); n = n / np.linalg.norm(n)
    return P.disk_emitter(np.column_stack([u, v, -n if flip else n, center]), radiance)


@pytest.mark.parametrize("boundary", [P.BOUNDARY_AABB, P.BOUNDARY_SPHERE])
def test_capi_refusals(boundary):
    base = scenes.homogeneous_scene(w=8, h=8, boundary=boundary)                # the cube [-1, 1]^3 or the unit sphere
    disk = _disk_param([0, 2, 0], [0.5, 0, 0], [0, 0, 0.5])
    ball = P.sphere_emitter([0.3, 2.4, 0.2], 0.7, [1, 1, 1])
    dome = P.sphere_emitter([0.1, 0, 0], 3.0, [1, 1, 1], flip_normals=True)
    capi.validate_emitters(base.copy(emitters=[disk, ball, dome]))
    with pytest.raises(capi.MerError, match="straight rays"):
        capi.validate_emitters(base.copy(emitters=[ball], rif_mode=P.RIF_TRILINEAR))
    with pytest.raises(capi.MerError, match="index-matched"):
        capi.validate_emitters(base.copy(emitters=[disk], boundary_bsdf=P.BSDF_HDIELECTRIC))
    with pytest.raises(capi.MerError, match="sphere must be clear"):               # meets the shape
        capi.validate_emitters(base.copy(emitters=[P.sphere_emitter([0, 1.5, 0], 0.7, [1, 1, 1])]))
    with pytest.raises(capi.MerError, match="sphere must be clear"):               # an outward sphere around the shape: its emission never reaches it
        capi.validate_emitters(base.copy(emitters=[P.sphere_emitter([0.1, 0, 0], 3.0, [1, 1, 1])]))
    with pytest.raises(capi.MerError, match="sphere must be clear"):               # a flipped sphere that cuts the shape
        capi.validate_emitters(base.copy(emitters=[P.sphere_emitter([1.0, 0, 0], 1.5, [1, 1, 1], flip_normals=True)]))
    capi.validate_emitters(base.copy(emitters=[P.sphere_emitter([0.3, 2.4, 0.2], 0.7, [1, 1, 1], flip_normals=True)]))   # flipped and apart: dark, allowed
    with pytest.raises(capi.MerError, match="disk must lie outside"):
        capi.validate_emitters(base.copy(emitters=[_disk_param([0, 0.5, 0], [0.5, 0, 0], [0, 0, 0.5])]))
    with pytest.raises(capi.MerError, match="contains shear"):
        capi.validate_emitters(base.copy(emitters=[P.disk_emitter(np.array([[1, 0.3, 0, 0], [0, 1, 0, 2.0], [0, 0, 1, 0]]), [1, 1, 1])]))
    with pytest.raises(capi.MerError, match="non-uniform scale"):
        capi.validate_emitters(base.copy(emitters=[_disk_param([0, 2, 0], [0.5, 0, 0], [0, 0, 0.4])]))
    squashed = P.sphere_emitter([0.3, 2.4, 0.2], 0.7, [1, 1, 1]); squashed["to_world"][1, 1] = 0.5
    with pytest.raises(capi.MerError, match="non-uniform scale"):
        capi.validate_emitters(base.copy(emitters=[squashed]))
    with pytest.raises(capi.MerError, match="cannot be combined"):
        capi.validate_emitters(base.copy(emitters=[disk, P.point_emitter([0, 3, 0], [1, 1, 1])]))
    capi.validate_emitters(base.copy(emitters=[ball, P.point_emitter([0, 0.2, 0], [1, 1, 1])]))


def test_disk_placement_against_the_sphere_is_exact_and_against_the_cube_conservative():
    ball = scenes.homogeneous_scene(w=8, h=8, boundary=P.BOUNDARY_SPHERE)
    # a disk of radius 1 in the plane y = 0.8 centred at x = 1.55: its rim comes within hypot(0.55, 0.8) = 0.971 of the centre -- inside
    with pytest.raises(capi.MerError, match="disk must lie outside"):
        capi.validate_emitters(ball.copy(emitters=[_disk_param([1.55, 0.8, 0], [1, 0, 0], [0, 0, 1])]))
    capi.validate_emitters(ball.copy(emitters=[_disk_param([1.65, 0.8, 0], [1, 0, 0], [0, 0, 1])]))     # hypot(0.65, 0.8) = 1.03: outside
    # against the cube the circumscribed square decides: rotated by 45 degrees about y its corner reaches the cube although the disk does not
    cube = scenes.homogeneous_scene(w=8, h=8)
    s = np.sqrt(0.5)
    capi.validate_emitters(cube.copy(emitters=[_disk_param([2.2, 0.5, 0], [1, 0, 0], [0, 0, 1])]))       # square x in [1.2, 3.2]: clear
    with pytest.raises(capi.MerError, match="disk must lie outside"):
        capi.validate_emitters(cube.copy(emitters=[_disk_param([2.2, 0.5, 0], [s, 0, s], [-s, 0, s])]))  # corner at x = 2.2 - 1.414 < 1; the disk ends at 1.2


def test_scene_desc_carries_the_shapes_and_the_abi_keeps_its_size():
    p = scenes.homogeneous_scene(w=8, h=8, emitters=[P.sphere_emitter([0.3, 2.4, 0.2], 0.7, [1, 2, 3], 2.0), _disk_param([0, 2, 0], [0.5, 0, 0], [0, 0, 0.5], (4, 5, 6))])

    class _NoGpu(capi.Context):
        def __init__(self):
            pass
    s = _NoGpu().scene_desc(p)
    assert s.n_emitters == 2 and [s.emitters[i].type for i in range(2)] == [6, 5]
    assert list(s.emitters[0].radiance) == [1, 2, 3] and s.emitters[0].sampling_weight == 2.0 and list(s.emitters[1].radiance) == [4, 5, 6]
    assert np.allclose(np.array(list(s.emitters[0].to_world)).reshape(3, 4)[:, 3], [0.3, 2.4, 0.2])
    assert ctypes.sizeof(capi.EmitterDesc) == 92
    assert capi.lib().mer_abi_version() == 3
    assert hasattr(capi.lib(), "mer_area_direct") and hasattr(capi.lib(), "mer_area_hit")
