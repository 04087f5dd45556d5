"""`<emitter type="envmap">` in the XML host (src/emitters/envmap.cpp:103-187): flattening into an emitter-list entry, every refusal, and the
image readers -- .pfm and uncompressed scan-line OpenEXR with FLOAT or HALF channels -- on files written here.  No GPU."""
import os
import struct
import numpy as np
import pytest
from mitsubaer_amd import host, params as P
from tests.test_host_multi_emitter import _scene, _point
from tests.envmap64 import sun_and_gradient

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_pfm(path, rgb, big_endian=False):
    h, w, _ = rgb.shape
    with open(path, "wb") as f:
        f.write(b"PF\n%d %d\n%s\n" % (w, h, b"1.0" if big_endian else b"-1.0"))
        f.write(np.ascontiguousarray(rgb[::-1], ">f4" if big_endian else "<f4").tobytes())


def _write_exr(path, rgb, half=False, extra_channel=False):
    """OpenEXR 2, one part, scan lines, no compression; channels in alphabetical order (A?, B, G, R), HALF (1) or FLOAT (2)"""
    h, w, _ = rgb.shape
    t, dt = (1, "<f2") if half else (2, "<f4")
    names = (["A"] if extra_channel else []) + ["B", "G", "R"]
    planes = {"A": np.ones((h, w)), "B": rgb[..., 2], "G": rgb[..., 1], "R": rgb[..., 0]}
    def attr(name, typ, data):
        return name.encode() + b"\0" + typ.encode() + b"\0" + struct.pack("<i", len(data)) + data
    ch = b"".join(n.encode() + b"\0" + struct.pack("<i", t) + b"\0\0\0\0" + struct.pack("<ii", 1, 1) for n in names) + b"\0"
    hdr = struct.pack("<ii", 20000630, 2) + attr("channels", "chlist", ch) + attr("compression", "compression", b"\0")
    hdr += attr("dataWindow", "box2i", struct.pack("<4i", 0, 0, w - 1, h - 1)) + attr("displayWindow", "box2i", struct.pack("<4i", 0, 0, w - 1, h - 1))
    hdr += attr("lineOrder", "lineOrder", b"\0") + attr("pixelAspectRatio", "float", struct.pack("<f", 1.0))
    hdr += attr("screenWindowCenter", "v2f", struct.pack("<2f", 0, 0)) + attr("screenWindowWidth", "float", struct.pack("<f", 1.0)) + b"\0"
    lines = [b"".join(np.ascontiguousarray(planes[n][y], dt).tobytes() for n in names) for y in range(h)]
    base = len(hdr) + 8 * h
    offs, pos = [], base
    for ln in lines:
        offs.append(pos); pos += 8 + len(ln)
    with open(path, "wb") as f:
        f.write(hdr + struct.pack("<%dQ" % h, *offs))
        for y, ln in enumerate(lines):
            f.write(struct.pack("<iI", y, len(ln)) + ln)


def _env(fn="sky.pfm", extra=""):
    return '<emitter type="envmap"><string name="filename" value="%s"/>%s</emitter>' % (fn, extra)


IMG = sun_and_gradient(12, 20)


@pytest.fixture
def sky(tmp_path):
    _write_pfm(str(tmp_path / "sky.pfm"), IMG)
    return tmp_path


@pytest.mark.parametrize("kind", ["pfm_le", "pfm_be", "exr_float", "exr_half", "exr_float_with_alpha", "exr_written_by_the_host"])
def test_image_round_trip(tmp_path, kind):
    f = str(tmp_path / ("m.pfm" if kind.startswith("pfm") else "m.exr"))
    expect = IMG
    if kind == "pfm_le":
        _write_pfm(f, IMG)
    elif kind == "pfm_be":
        _write_pfm(f, IMG, big_endian=True)
    elif kind == "exr_float":
        _write_exr(f, IMG)
    elif kind == "exr_half":
        _write_exr(f, IMG, half=True); expect = IMG.astype(np.float16).astype(np.float32)
    elif kind == "exr_float_with_alpha":
        _write_exr(f, IMG, extra_channel=True)
    else:
        host.write_exr(f, IMG)
    np.testing.assert_array_equal(host.read_envmap_image(f), expect)


def test_envmap_flattens_into_a_list_entry(sky):
    extra = ('<float name="scale" value="2.5"/><float name="samplingWeight" value="3"/><boolean name="cache" value="false"/>'
             '<transform name="toWorld"><rotate y="1" angle="90"/><translate x="4" y="5" z="6"/></transform>')
    d, _ = host.flatten_xml(_scene(sky, _env(extra=extra) + _point(0.1, 0.2, 0.3)))
    assert d.n_emitters == 2 and list(d.env_radiance) == [0, 0, 0]
    e = d.emitters[0]
    assert e.type == P.EMITTER_ENVMAP and e.envmap == 0 and e.env_scale == 2.5 and e.sampling_weight == 3.0
    M = np.array(e.to_world).reshape(3, 4)
    np.testing.assert_allclose(M[:, :3], [[0, 0, 1], [0, 1, 0], [-1, 0, 0]], atol=1e-6)
    assert d.emitters[1].type == P.EMITTER_POINT


@pytest.mark.parametrize("extra, match", [
    ('<float name="gamma" value="2.2"/>', "gamma"),
    ('<float name="scale" value="-1"/>', "scale"),
    ('<float name="intensityScale" value="2"/>', "deprecated"),
    ('<transform name="toWorld"><scale x="2" y="1" z="1"/></transform>', "rotation"),
    ('<transform name="toWorld"><scale x="-1" y="1" z="1"/></transform>', "rotation"),
    ('<float name="samplingWeight" value="0"/>', "samplingWeight"),
])
def test_xml_refusals(sky, extra, match):
    with pytest.raises(host.HostError, match=match):
        host.flatten_xml(_scene(sky, _env(extra=extra)))


def test_missing_file_and_other_formats(sky):
    with pytest.raises(host.HostError, match="could not be found"):
        host.flatten_xml(_scene(sky, _env("nothing.exr")))
    (sky / "sky.hdr").write_bytes(b"#?RADIANCE\n")
    with pytest.raises(host.HostError, match="not a .pfm or OpenEXR"):
        host.flatten_xml(_scene(sky, _env("sky.hdr")))
    _write_pfm(str(sky / "black.pfm"), np.zeros((4, 8, 3), np.float32))
    host.flatten_xml(_scene(sky, _env("black.pfm")))          # configure()'s refusal of a black map runs where the tables are built (mer_envmap_upload)


def test_one_environment_emitter(sky):
    with pytest.raises(host.HostError, match="only contain one environment emitter"):
        host.flatten_xml(_scene(sky, _env() + _env()))
    with pytest.raises(host.HostError, match="only contain one environment emitter"):
        host.flatten_xml(_scene(sky, '<emitter type="constant"/>' + _env()))
    with pytest.raises(host.HostError, match="only contain one environment emitter"):
        host.flatten_xml(_scene(sky, _env() + '<emitter type="constant"/>'))


def test_example_scene_flattens(tmp_path):
    import subprocess, shutil, sys
    shutil.copy(os.path.join(ROOT, "scenes", "cfg_envmap.xml"), str(tmp_path / "cfg_envmap.xml"))
    subprocess.check_call([sys.executable, os.path.join(ROOT, "scenes", "make_envmap.py"), str(tmp_path / "sky.pfm")])
    d, spp = host.flatten_xml(str(tmp_path / "cfg_envmap.xml"), {"samples": 4})
    assert d.n_emitters == 1 and d.emitters[0].type == P.EMITTER_ENVMAP and spp == 4
