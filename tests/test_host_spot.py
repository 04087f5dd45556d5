"""Spot emitters without a GPU: the XML vocabulary of `spot` (src/emitters/spot.cpp:66-77), its place in the emitter list of
mer_scene_desc, the refusals of the host parser and of params / capi, and the layout of the ctypes mirror."""
import ctypes
import os
import subprocess
import numpy as np
import pytest
from mitsubaer_amd import host, params as P, capi
from tests import scenes
from tests.test_host_multi_emitter import _scene, _point, _rect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _spot(transform='<lookat origin="0, 3, 0" target="0, 0, 0" up="0, 0, 1"/>', extra=""):
    return '<emitter type="spot"><transform name="toWorld">%s</transform>%s</emitter>' % (transform, extra)


def _entries(d):
    return [d.emitters[i] for i in range(d.n_emitters)]


def test_lookat_spot_with_defaults_is_a_list_entry(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, _spot()))
    assert d.n_emitters == 1                                                   # always the list form, even alone
    assert list(d.point_intensity) == [0, 0, 0]
    e = _entries(d)[0]
    assert e.type == P.EMITTER_SPOT
    m = np.array(list(e.to_world)).reshape(3, 4)
    assert np.allclose(m[:, 3], [0, 3, 0]) and np.allclose(m[:, 2], [0, -1, 0], atol=1e-6)     # lookAt: z axis toward the target
    assert np.allclose(list(e.position), [0, 3, 0])
    assert np.allclose(list(e.intensity), [1, 1, 1])                          # intensity defaults to 1 (not D65)
    assert e.cutoff_angle_deg == 20.0 and e.beam_width_deg == 15.0 and e.sampling_weight == 1.0


def test_spot_properties_and_weights(tmp_path):
    extra = ('<spectrum name="intensity" value="4, 2, 1"/><float name="cutoffAngle" value="30"/><float name="beamWidth" value="12.5"/>'
             '<float name="samplingWeight" value="2.5"/><spectrum name="texture" value="0.3"/>')
    tr = '<rotate x="1" y="0" z="0" angle="90"/><translate x="0.5" y="2.5" z="-0.25"/>'
    d, _ = host.flatten_xml(_scene(tmp_path, _spot(tr, extra) + _point(0.1, 0.2, 0.3, weight=0.5) + _spot()))
    e = _entries(d)
    assert [x.type for x in e] == [P.EMITTER_SPOT, P.EMITTER_POINT, P.EMITTER_SPOT]
    assert np.allclose(list(e[0].intensity), [4, 2, 1]) and e[0].cutoff_angle_deg == 30.0 and e[0].beam_width_deg == 12.5
    assert e[0].sampling_weight == 2.5 and e[1].sampling_weight == 0.5
    m = np.array(list(e[0].to_world)).reshape(3, 4)
    assert np.allclose(m[:, 3], [0.5, 2.5, -0.25]) and np.allclose(m[:, 2], [0, -1, 0], atol=1e-6)   # rotate x by 90: z -> -y
    assert np.allclose(list(e[1].position), [0.1, 0.2, 0.3])


def test_default_beam_is_three_quarters_of_the_cutoff(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, _spot(extra='<float name="cutoffAngle" value="33"/>')))
    assert _entries(d)[0].beam_width_deg == np.float32(33) * np.float32(0.75)


@pytest.mark.parametrize("extra, match", [
    ('<float name="cutoffAngle" value="20"/><float name="beamWidth" value="25"/>', "beamWidth"),
    ('<float name="cutoffAngle" value="-5"/><float name="beamWidth" value="0"/>', "non-negative"),
    ('<float name="cutoffAngle" value="190"/>', "180"),
    ('<texture type="bitmap" name="texture"><string name="filename" value="a.png"/></texture>', "texture"),
])
def test_xml_refusals(tmp_path, extra, match):
    with pytest.raises(host.HostError, match=match):
        host.flatten_xml(_scene(tmp_path, _spot(extra=extra)))


def test_xml_refuses_a_singular_frame(tmp_path):
    with pytest.raises(host.HostError, match="singular"):
        host.flatten_xml(_scene(tmp_path, _spot('<scale x="1" y="1" z="0"/>')))


def test_xml_refuses_a_spot_inside_a_rough_shape_and_beside_a_rectangle(tmp_path):
    rough = '<shape type="cube"><ref name="interior" id="m"/><bsdf type="hroughdielectric"/></shape>'
    with pytest.raises(host.HostError, match="spot emitter must lie outside"):
        host.flatten_xml(_scene(tmp_path, _spot('<translate x="0.1" y="0" z="0"/>'), shape=rough))
    host.flatten_xml(_scene(tmp_path, _spot(), shape=rough))                  # outside: accepted
    with pytest.raises(host.HostError, match="cannot be combined with an area emitter"):
        host.flatten_xml(_scene(tmp_path, _rect(2.5, 90) + _spot('<lookat origin="3, 0, 0" target="0, 0, 0" up="0, 1, 0"/>')))


def test_xml_counts_spots_toward_the_cap(tmp_path):
    with pytest.raises(host.HostError, match="At most 32"):
        host.flatten_xml(_scene(tmp_path, _spot() * 20 + _point(0, 0, 0) * 13))


def test_example_scene_parses():
    d, spp = host.flatten_xml(os.path.join(ROOT, "scenes", "cfg_spot.xml"), {"samples": "4"})
    e = _entries(d)
    assert any(x.type == P.EMITTER_SPOT for x in e) and spp > 0
    for x in e:
        if x.type == P.EMITTER_SPOT:
            assert 0 <= x.beam_width_deg < x.cutoff_angle_deg <= 180


def test_params_spot_emitter():
    e = P.spot_emitter(np.eye(4), [1, 2, 3])
    assert e["type"] == P.EMITTER_SPOT and e["cutoff_deg"] == 20.0 and e["beam_deg"] == 15.0 and e["sampling_weight"] == 1.0
    e = P.spot_emitter(np.eye(4)[:3], [1, 1, 1], cutoff_deg=40, beam_deg=10, weight=3)
    assert e["beam_deg"] == 10.0 and e["sampling_weight"] == 3.0
    for kw, match in [(dict(cutoff_deg=20, beam_deg=25), "beamWidth"), (dict(cutoff_deg=-1, beam_deg=0), "non-negative"),
                      (dict(cutoff_deg=float("nan")), "finite"), (dict(cutoff_deg=181, beam_deg=10), "180")]:
        with pytest.raises(ValueError, match=match):
            P.spot_emitter(np.eye(4), [1, 1, 1], **kw)
    with pytest.raises(ValueError, match="singular"):
        P.spot_emitter(np.diag([1.0, 0.0, 1.0, 1.0]), [1, 1, 1])
    with pytest.raises(ValueError, match="finite"):
        P.spot_emitter(np.full((4, 4), np.inf), [1, 1, 1])


def test_capi_validation_of_spot_entries():
    up = np.array([[1.0, 0, 0, 0], [0, 0, -1, 3.0], [0, 1, 0, 0]])
    inside = np.array([[1.0, 0, 0, 0.1], [0, 1, 0, 0], [0, 0, 1, 0]])
    rough = dict(boundary_bsdf=P.BSDF_HROUGHDIELECTRIC, rough_distribution=P.MICROFACET_GGX, rough_alpha=0.2)
    capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, emitters=[P.spot_emitter(up, [1, 1, 1])]))
    with pytest.raises(capi.MerError, match="spot emitter must lie outside"):
        capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, emitters=[P.spot_emitter(inside, [1, 1, 1])], **rough))
    with pytest.raises(capi.MerError, match="cannot be combined with an area emitter"):
        capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, emitters=[P.spot_emitter(up, [1, 1, 1]), P.area_emitter(
            np.array([[1.0, 0, 0, 0], [0, 0, -1, -2.5], [0, 1.0, 0, 0]]), [1, 1, 1])]))
    e = P.spot_emitter(up, [1, 1, 1]); e["beam_deg"] = 30.0                     # edited past spot_emitter's own check
    with pytest.raises(capi.MerError, match="beamWidth"):
        capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, emitters=[e]))
    with pytest.raises(capi.MerError, match="at most 32"):
        capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, emitters=[P.spot_emitter(up, [1, 1, 1])] * 33))


def test_emitter_struct_matches_header(tmp_path):
    src = '#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu\\n", sizeof(mer_emitter), offsetof(mer_emitter, cutoff_angle_deg));return 0;}\n'
    c = tmp_path / "s.c"; c.write_text(src)
    exe = str(tmp_path / "s")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)])
    size, off = map(int, subprocess.check_output([exe]).split())
    assert ctypes.sizeof(capi.EmitterDesc) == size
    e = capi.EmitterDesc(); e.cutoff_angle_deg = 7.0
    assert (ctypes.c_float * (size // 4)).from_buffer(e)[off // 4] == 7.0          # the field sits where the header puts it
    assert P.EMITTER_SPOT == 3
