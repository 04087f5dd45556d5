"""The time-resolved fluence grid's interface without a GPU: the header declares the two new entry points and both libraries export them,
the ctypes mirror of mer_fluence_time_desc has the C compiler's size and offsets, validate_fluence_time refuses what
mer_fluence_time_create refuses, with its messages, and `mer_render --time-resolved` refuses a missing --fluence=, a VOL output and
several GPUs while it still parses its arguments, and a film without decomposition = transient before it touches a device."""
import ctypes
import os
import re
import subprocess
import tempfile
import pytest
from mitsubaer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["mer_fluence_time_create", "mer_fluence_time_read"]
MER_RENDER = os.path.join(ROOT, "mitsubaer_amd", "mer_render")
SCENE = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
BOX = ((-1, -1, -1), (1, 1, 1))


def test_header_declares_and_libraries_export_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mer.h")).read(), flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % f, txt), f
        assert f in capi.SYMBOLS
        assert hasattr(capi.lib(), f) and hasattr(capi.lib(capi.CHECK_LIB_PATH), f), f
    assert txt.index("} mer_shard;") < txt.index("mer_fluence_desc;") < txt.index("mer_fluence_time_desc;")
    assert "MER_ABI_VERSION 3" in txt


def test_desc_mirror_has_the_compilers_size_and_offsets():
    fields = ["res", "bmin", "bmax", "frames", "t_min", "t_bin", "reserved"]
    src = ('#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(mer_fluence_time_desc));\n'
           + "".join('printf(" %%zu", offsetof(mer_fluence_time_desc, %s));\n' % f for f in fields) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        size, *offsets = map(int, subprocess.check_output([os.path.join(d, "t")]).split())
    assert ctypes.sizeof(capi.FluenceTimeDesc) == size == 52
    assert [getattr(capi.FluenceTimeDesc, f).offset for f in fields] == offsets == [0, 12, 24, 36, 40, 44, 48]


def _desc(res=(8, 8, 8), frames=8, t_min=1.9, t_bin=0.35, reserved=0, box=BOX):
    d = capi.fluence_time_desc(res, box[0], box[1], frames, t_min, t_bin)
    d.reserved = reserved
    return d


@pytest.mark.parametrize("kw,msg", [
    (dict(frames=0), "frames must lie in 1 ... 4096"),
    (dict(frames=4097), "frames must lie in 1 ... 4096"),
    (dict(t_bin=0.0), "t_bin must be finite and greater than 0"),
    (dict(t_bin=-0.35), "t_bin must be finite and greater than 0"),
    (dict(t_bin=float("nan")), "t_bin must be finite and greater than 0"),
    (dict(t_min=float("inf")), "t_min must be finite"),
    (dict(reserved=1), "reserved must be 0"),
    (dict(res=(1024, 1024, 64), frames=3), "more than 2\\^27 cells x frames"),
    # the box checks of mer_fluence_create, under the new prefix
    (dict(res=(0, 8, 8)), "res must lie in 1 ... 1024"),
    (dict(box=((-1, 1, -1), (1, 1, 1))), "bmin must be below bmax"),
    (dict(box=((-1, -1, -1), (1, float("nan"), 1))), "must be finite"),
    (dict(res=(1024, 1024, 129), frames=1), "more than 2\\^27 cells"),
])
def test_validate_fluence_time_refuses(kw, msg):
    with pytest.raises(capi.MerError, match="^mer_fluence_time_create: .*" + msg):
        capi.validate_fluence_time(_desc(**kw))


def test_validate_fluence_time_accepts():
    capi.validate_fluence_time(_desc())
    capi.validate_fluence_time(_desc(res=(1, 1, 1), frames=1, t_min=-3.0, t_bin=1e-3))
    capi.validate_fluence_time(_desc(res=(1024, 1024, 64), frames=2))          # exactly 2^27 keys
    capi.validate_fluence_time(_desc(res=(32, 32, 32), frames=4096))           # exactly 2^27 keys, the film's cap of frames


def _run(*args):
    r = subprocess.run([MER_RENDER, *args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


def test_mer_render_refuses_time_resolved_alone():
    rc, err = _run("--time-resolved", "-D", "samples=2", "-D", "tMin=4", "-D", "tMax=9", "-D", "tRes=0.5", "-D", "medium=homogeneous", SCENE)
    assert rc == 2 and "--time-resolved needs --fluence=NX,NY,NZ" in err, (rc, err)


@pytest.mark.parametrize("out", ["phi.vol", "phi.pfm", "phi"])
def test_mer_render_refuses_time_resolved_into_anything_but_npy(out):
    rc, err = _run("--fluence=8,8,8", "--time-resolved", "-o", out, SCENE)
    assert rc == 2 and "--time-resolved writes a .npy file" in err, (rc, err)
    assert not os.path.exists(out)


@pytest.mark.parametrize("multi", [["--gpus", "2"], ["--devices", "0,0"]])
def test_mer_render_refuses_time_resolved_on_several_gpus(multi):
    rc, err = _run("--fluence=8,8,8", "--time-resolved", *multi, SCENE)
    assert rc == 2 and "--fluence runs on one GPU" in err, (rc, err)


def test_mer_render_refuses_time_resolved_without_a_transient_film(tmp_path):
    """the window comes from the film: the laser scene with decomposition = none is refused by name, before any device is touched"""
    xml = open(SCENE).read()
    assert xml.count('<string name="decomposition" value="transient"/>') == 1
    scene = tmp_path / "laser_steady.xml"
    scene.write_text(xml.replace('<string name="decomposition" value="transient"/>', '<string name="decomposition" value="none"/>'))
    rc, err = _run("--fluence=8,8,8", "--time-resolved", "-o", str(tmp_path / "phi.npy"), "-D", "samples=2", "-D", "tMin=4", "-D", "tMax=9", "-D", "tRes=0.5",
                   "-D", "medium=homogeneous", str(scene))
    assert rc == 1 and "decomposition = transient" in err, (rc, err)
    assert not (tmp_path / "phi.npy").exists()
