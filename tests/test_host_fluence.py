"""The fluence grid's interface without a GPU: the header declares the five entry points and both libraries export them, the ctypes mirror
of mer_fluence_desc has the C compiler's size, validate_fluence refuses what mer_fluence_create refuses, with its messages, and
`mer_render --fluence` refuses a malformed value and several GPUs while it still parses its arguments, and a scene whose integrator is
not `ptracer` before it touches a device."""
import ctypes
import os
import re
import subprocess
import tempfile
import pytest
from mitsubaer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["mer_fluence_create", "mer_fluence_clear", "mer_fluence_destroy", "mer_render_fluence", "mer_fluence_read"]
MER_RENDER = os.path.join(ROOT, "mitsubaer_amd", "mer_render")
SCENE = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")


def test_header_declares_and_libraries_export_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mer.h")).read(), flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % f, txt), f
        assert f in capi.SYMBOLS
        assert hasattr(capi.lib(), f) and hasattr(capi.lib(capi.CHECK_LIB_PATH), f), f
    # the new struct stands after mer_shard: the block before `} mer_scene_desc;` stays the last `typedef struct {` in front of it
    assert txt.index("} mer_shard;") < txt.index("mer_fluence_desc;")
    assert "MER_ABI_VERSION 3" in txt


def test_desc_mirror_has_the_compilers_size():
    src = '#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu\\n", sizeof(mer_fluence_desc), offsetof(mer_fluence_desc, bmin), offsetof(mer_fluence_desc, bmax), sizeof(mer_fluence));return 0;}\n'
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        size, o1, o2, hs = map(int, subprocess.check_output([os.path.join(d, "t")]).split())
    assert ctypes.sizeof(capi.FluenceDesc) == size == 36
    assert capi.FluenceDesc.bmin.offset == o1 and capi.FluenceDesc.bmax.offset == o2 and hs == 4


@pytest.mark.parametrize("res,bmin,bmax,msg", [
    ((0, 8, 8), (-1, -1, -1), (1, 1, 1), "res must lie in 1 ... 1024"),
    ((8, -3, 8), (-1, -1, -1), (1, 1, 1), "res must lie in 1 ... 1024"),
    ((8, 8, 1025), (-1, -1, -1), (1, 1, 1), "res must lie in 1 ... 1024"),
    ((1024, 1024, 129), (-1, -1, -1), (1, 1, 1), "more than 2\\^27 cells"),
    ((8, 8, 8), (-1, 1, -1), (1, 1, 1), "bmin must be below bmax"),
    ((8, 8, 8), (-1, -1, 2), (1, 1, 1), "bmin must be below bmax"),
    ((8, 8, 8), (float("nan"), -1, -1), (1, 1, 1), "must be finite"),
    ((8, 8, 8), (-1, -1, -1), (1, float("inf"), 1), "must be finite"),
])
def test_validate_fluence_refuses(res, bmin, bmax, msg):
    with pytest.raises(capi.MerError, match="mer_fluence_create: .*" + msg):
        capi.validate_fluence(capi.fluence_desc(res, bmin, bmax))


def test_validate_fluence_accepts():
    capi.validate_fluence(capi.fluence_desc((1, 1, 1), (-1, -1, -1), (1, 1, 1)))
    capi.validate_fluence(capi.fluence_desc((1024, 1024, 128), (-1, -0.5, -1), (0.5, 1, 0.25)))       # exactly 2^27 cells


def _run(*args):
    r = subprocess.run([MER_RENDER, *args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


@pytest.mark.parametrize("value", ["--fluence", "--fluence=", "--fluence=8,8", "--fluence=8,8,8,8", "--fluence=8,x,8", "--fluence=8,,8", "--fluence=0,8,8",
                                   "--fluence=8,8,1025", "--fluence=1024,1024,129", "--fluence=8,8,-8", "--fluence=8,8,8 "])
def test_mer_render_refuses_a_malformed_fluence_value(value):
    rc, err = _run(value, SCENE)
    assert rc == 2 and "--fluence=NX,NY,NZ expects three cell counts" in err, (rc, err)


@pytest.mark.parametrize("multi", [["--gpus", "2"], ["--devices", "0,0"]])
def test_mer_render_refuses_fluence_on_several_gpus(multi):
    rc, err = _run("--fluence=8,8,8", *multi, SCENE)
    assert rc == 2 and "--fluence runs on one GPU" in err, (rc, err)
    rc, err = _run(*multi, "--fluence=8,8,8", SCENE)
    assert rc == 2 and "--fluence runs on one GPU" in err, (rc, err)


def test_mer_render_refuses_fluence_for_a_camera_path_scene():
    """the grid is recorded from light paths: a volpath scene is refused by name, before any device is touched"""
    rc, err = _run("--fluence=8,8,8", "-D", "samples=2", os.path.join(ROOT, "scenes", "cfg1_homogeneous_box.xml"))
    assert rc == 1 and "integrator must be \"ptracer\"" in err, (rc, err)
