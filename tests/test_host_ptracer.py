"""Host side of light tracing (no GPU): the `ptracer` integrator and the `collimated` emitter in the scene XML, the example scene, the
refusals of the host parser and of capi.validate_*, and the layout of the fields the scene desc gained."""
import ctypes
import os
import subprocess
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEAM = ('<emitter type="collimated"><transform name="toWorld"><lookat origin="0.2, 0.1, -3" target="0.2, 0.1, 0" up="0, 1, 0"/></transform>'
        '<spectrum name="power" value="5, 6, 7"/>{extra}</emitter>')
PTRACER = '<integrator type="ptracer"><integer name="maxDepth" value="6"/><integer name="rrDepth" value="4"/>{extra}</integrator>'


def _scene(tmp_path, integrator=PTRACER.format(extra=""), emitters=BEAM.format(extra=""), sensor="perspective", shape_extra="", medium_extra=""):
    xml = ('<scene version="0.5.0">' + integrator +
           '<medium type="homogeneous" id="m"><spectrum name="sigmaS" value="1"/><spectrum name="sigmaA" value="0.2"/>' + medium_extra +
           '<phase type="hg"><float name="g" value="0.5"/></phase></medium>'
           '<shape type="cube"><ref name="interior" id="m"/>' + shape_extra + '</shape>' + emitters +
           '<sensor type="' + sensor + '"><float name="fov" value="40"/><transform name="toWorld"><lookat origin="-3, 0, 0" target="0, 0, 0" up="0, 1, 0"/></transform>'
           '<sampler type="independent"><integer name="sampleCount" value="4"/></sampler>'
           '<film type="hdrfilm"><integer name="width" value="24"/><integer name="height" value="20"/><rfilter type="box"/></film></sensor></scene>')
    f = tmp_path / "scene.xml"
    f.write_text(xml)
    return str(f)


def test_ptracer_and_collimated_flatten(tmp_path):
    d, spp = host.flatten_xml(_scene(tmp_path, PTRACER.format(extra='<integer name="granularity" value="1000"/><boolean name="bruteForce" value="false"/>'),
                                     BEAM.format(extra='<float name="samplingWeight" value="2.5"/>')))
    assert spp == 4 and d.integrator == P.INTEGRATOR_PTRACER == 1 and d.integrator_reserved == 0
    assert d.max_depth == 6 and d.rr_depth == 4
    assert d.n_emitters == 1
    e = d.emitters[0]
    assert e.type == P.EMITTER_COLLIMATED == 7 and list(e.intensity) == [5, 6, 7] and e.sampling_weight == 2.5
    m = np.array(list(e.to_world)).reshape(3, 4)
    np.testing.assert_allclose(m[:, 3], [0.2, 0.1, -3], atol=1e-6)             # the origin: the translation column
    np.testing.assert_allclose(m[:, 2], [0, 0, 1], atol=1e-6)                  # the direction: the image of (0, 0, 1)
    assert all(v == 0 for v in d.env_radiance) and all(v == 0 for v in d.point_intensity)
    # a point emitter under ptracer is a list entry too (the legacy fields are volpath's)
    d, _ = host.flatten_xml(_scene(tmp_path, emitters='<emitter type="point"><point name="position" x="0.1" y="0" z="0"/></emitter>'))
    assert d.n_emitters == 1 and d.emitters[0].type == P.EMITTER_POINT and all(v == 0 for v in d.point_intensity)
    # volpath scenes keep integrator = 0
    d, _ = host.flatten_xml(os.path.join(ROOT, "scenes", "cfg_spot.xml"), {"samples": "2"})
    assert d.integrator == P.INTEGRATOR_VOLPATH == 0 and d.integrator_reserved == 0


def test_example_scene_flattens():
    defs = {"samples": "4", "tMin": "4", "tMax": "9", "tRes": "0.05"}
    path = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
    d, spp = host.flatten_xml(path, dict(defs, medium="homogeneous"))
    assert spp == 4 and d.integrator == P.INTEGRATOR_PTRACER and d.n_emitters == 1 and d.emitters[0].type == P.EMITTER_COLLIMATED
    assert d.decomposition == P.DECOMPOSITION_TRANSIENT and d.rif_mode == P.RIF_CONST and d.sigma_mode == P.SIGMA_HOMOGENEOUS
    assert abs(d.min_bound - 4) < 1e-6 and abs(d.max_bound - 9) < 1e-6 and abs(d.bin_width - 0.05) < 1e-6
    d, _ = host.flatten_xml(path, dict(defs, medium="refractive"))
    assert d.rif_mode == P.RIF_ACOUSTIC and d.stepper == P.STEP_RK4 and d.ac_mode == 1 and d.integrator == P.INTEGRATOR_PTRACER
    with pytest.raises(host.HostError, match="nosuch"):
        host.flatten_xml(path, dict(defs, medium="nosuch"))


def test_host_refusals(tmp_path):
    with pytest.raises(host.HostError, match="bruteForce"):
        host.flatten_xml(_scene(tmp_path, PTRACER.format(extra='<boolean name="bruteForce" value="true"/>')))
    with pytest.raises(host.HostError, match="only 'volpath'"):
        host.flatten_xml(_scene(tmp_path, '<integrator type="bdpt"/>'))
    scaled = ('<emitter type="collimated"><transform name="toWorld"><scale value="2"/><translate x="0" y="0" z="-3"/></transform></emitter>')
    with pytest.raises(host.HostError, match="Scale factors in the emitter-to-world transformation are not allowed!"):
        host.flatten_xml(_scene(tmp_path, emitters=scaled))
    with pytest.raises(host.HostError, match="no camera path"):
        host.flatten_xml(_scene(tmp_path, '<integrator type="volpath"/>'))
    with pytest.raises(host.HostError, match="constant and envmap emitters"):
        host.flatten_xml(_scene(tmp_path, emitters=BEAM.format(extra="") + '<emitter type="constant"/>'))
    rect = ('<shape type="rectangle"><transform name="toWorld"><translate x="0" y="0" z="3"/></transform><emitter type="area"/></shape>')
    with pytest.raises(host.HostError, match="area emitters"):
        host.flatten_xml(_scene(tmp_path, emitters=BEAM.format(extra="") + rect))
    with pytest.raises(host.HostError, match="no emitter"):
        host.flatten_xml(_scene(tmp_path, emitters=""))
    with pytest.raises(host.HostError, match="perspective sensor only"):
        host.flatten_xml(_scene(tmp_path, sensor="orthographic"))
    with pytest.raises(host.HostError, match="negative|non-negative"):
        host.flatten_xml(_scene(tmp_path, emitters=BEAM.format(extra="").replace("5, 6, 7", "-1")))


def _beam(**kw):
    return P.collimated_emitter(P.look_at([0.2, 0.1, -3], [0.2, 0.1, 0], [0, 1, 0]), [5, 5, 5], **kw)


def _base(**kw):
    kw.setdefault("env_radiance", [0, 0, 0])
    kw.setdefault("integrator", P.INTEGRATOR_PTRACER)
    kw.setdefault("emitters", [_beam()])
    return scenes.homogeneous_scene(w=8, h=8, **kw)


def test_capi_refusals_without_a_device():
    capi.validate_integrator(_base()); capi.validate_emitters(_base())
    with pytest.raises(capi.MerError, match="unknown integrator"):
        capi.validate_integrator(_base(integrator=2))
    with pytest.raises(capi.MerError, match="no camera path"):
        capi.validate_emitters(_base(integrator=P.INTEGRATOR_VOLPATH))
    with pytest.raises(ValueError, match="Scale factors"):
        P.collimated_emitter(np.diag([2.0, 2.0, 2.0, 1.0]), [1, 1, 1])
    e = _beam(); e["to_world"] = np.diag([1.0, 1.0, -1.0, 1.0])                  # a reflection, edited past collimated_emitter's own check
    with pytest.raises(capi.MerError, match="Scale factors"):
        capi.validate_emitters(_base(emitters=[e]))
    e = _beam(); e["power"] = [1, -1, 1]
    with pytest.raises(capi.MerError, match="non-negative"):
        capi.validate_emitters(_base(emitters=[e]))
    with pytest.raises(capi.MerError, match="samplingWeight"):
        capi.validate_emitters(_base(emitters=[_beam(sampling_weight=0.0)]))
    for kw, msg in [(dict(env_radiance=[1, 1, 1]), "env_radiance"), (dict(sensor=P.SENSOR_ORTHOGRAPHIC), "perspective sensor only"),
                    (dict(sensor=P.SENSOR_THINLENS, focus_distance=1.0), "perspective sensor only"),
                    (dict(boundary_bsdf=P.BSDF_HDIELECTRIC), "dielectric boundaries"), (dict(boundary=P.BOUNDARY_SDF), "signed-distance"),
                    (dict(emitters=[]), "no emitter"), (dict(point_intensity=[1, 1, 1], emitters=[]), "list entries"),
                    (dict(emission=[1, 0, 0]), "medium emission"),
                    (dict(emitters=[_beam(), P.area_emitter(np.array([[1.0, 0, 0, 0], [0, 0, -1, 2.5], [0, 1.0, 0, 0]]), [1, 1, 1])]), "area emitters"),
                    (dict(emitters=[P.envmap_emitter(np.ones((4, 8, 3), np.float32))]), "envmap"),
                    (dict(emitters=[P.spot_emitter(np.diag([2.0, 2.0, 2.0, 1.0]), [1, 1, 1])]), "free of scale"),
                    (dict(cam_to_world=2.0 * P.look_at([-3, 0, 0], [0, 0, 0], [0, 1, 0])), "rigid")]:
        with pytest.raises(capi.MerError, match=msg):
            capi.validate_integrator(_base(**kw))


def test_scene_desc_carries_the_new_fields(tmp_path):
    class _NoGpu(capi.Context):
        def __init__(self):
            pass
    s = _NoGpu().scene_desc(_base(emitters=[_beam(sampling_weight=3.0), P.point_emitter([0.1, 0, 0], [1, 1, 1])]))
    assert s.integrator == 1 and s.integrator_reserved == 0 and s.n_emitters == 2
    assert s.emitters[0].type == 7 and list(s.emitters[0].intensity) == [5, 5, 5] and s.emitters[0].sampling_weight == 3.0
    assert _NoGpu().scene_desc(scenes.homogeneous_scene(w=8, h=8)).integrator == 0
    src = ('#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %d %d %d\\n", sizeof(mer_scene_desc), sizeof(mer_emitter), '
           'offsetof(mer_scene_desc, integrator), offsetof(mer_scene_desc, emitters), MER_EMITTER_COLLIMATED, MER_INTEGRATOR_PTRACER, MER_ABI_VERSION);return 0;}\n')
    c = tmp_path / "s.c"; c.write_text(src)
    exe = str(tmp_path / "s")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)])
    size, esize, off, off_list, coll, ptr, abi = map(int, subprocess.check_output([exe]).split())
    assert ctypes.sizeof(capi.SceneDesc) == size and ctypes.sizeof(capi.EmitterDesc) == esize == 4 * (1 + 3 + 3 + 12 + 3 + 1)
    # two words in front of the list pointer, which stays 8-byte aligned: no padding before or after them
    assert capi.SceneDesc.integrator.offset == off and capi.SceneDesc.emitters.offset == off_list == off + 8 and off_list % 8 == 0
    assert off == capi.SceneDesc.area_radiance.offset + 12
    assert size == capi.SceneDesc.rough_distribution.offset + 12 and (coll, ptr, abi) == (7, 1, 3)
