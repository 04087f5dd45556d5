"""The exitance map's interface without a GPU: the header declares the five entry points and both libraries export them, the ctypes mirror
of mer_exitance_desc has the C compiler's size and offsets, validate_exitance refuses what mer_exitance_create refuses, with its messages,
and `mer_render --exitance` refuses by name what it is not built for while it still parses its arguments."""
import ctypes
import os
import re
import subprocess
import tempfile
import pytest
from mitsubaer_amd import capi, params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["mer_exitance_create", "mer_exitance_clear", "mer_exitance_destroy", "mer_render_exitance", "mer_exitance_read"]
MER_RENDER = os.path.join(ROOT, "mitsubaer_amd", "mer_render")
SCENE = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")


def test_header_declares_and_libraries_export_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mer.h")).read(), flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % f, txt), f
        assert f in capi.SYMBOLS
        assert hasattr(capi.lib(), f) and hasattr(capi.lib(capi.CHECK_LIB_PATH), f), f
    assert txt.index("} mer_shard;") < txt.index("mer_exitance_desc;") < txt.index("mer_exitance_create")
    assert "MER_ABI_VERSION 3" in txt


def test_desc_mirror_has_the_compilers_size_and_offsets():
    fields = ["boundary", "res", "frames", "t_min", "t_bin", "cos_min", "reserved"]
    src = ('#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(mer_exitance_desc));\n'
           + "".join('printf(" %%zu", offsetof(mer_exitance_desc, %s));\n' % f for f in fields) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        size, *offsets = map(int, subprocess.check_output([os.path.join(d, "t")]).split())
    assert ctypes.sizeof(capi.ExitanceDesc) == size == 32
    assert [getattr(capi.ExitanceDesc, f).offset for f in fields] == offsets == [0, 4, 12, 16, 20, 24, 28]


def _desc(boundary=P.BOUNDARY_AABB, res=(8, 8), frames=1, t_min=0.0, t_bin=0.0, cos_min=0.0, reserved=0):
    d = capi.exitance_desc(boundary, res, frames, t_min, t_bin, cos_min)
    d.reserved = reserved
    return d


@pytest.mark.parametrize("kw,msg", [
    (dict(boundary=P.BOUNDARY_SDF), "boundary must be the cube .* or the sphere"),
    (dict(boundary=-1), "boundary must be the cube .* or the sphere"),
    (dict(res=(0, 8)), "res must lie in 1 ... 4096"),
    (dict(res=(8, 4097)), "res must lie in 1 ... 4096"),
    (dict(frames=0, t_bin=0.5), "frames must lie in 1 ... 4096"),
    (dict(frames=4097, t_bin=0.5), "frames must lie in 1 ... 4096"),
    (dict(t_bin=-0.5), "t_bin must be finite and at least 0"),
    (dict(t_bin=float("nan")), "t_bin must be finite and at least 0"),
    (dict(t_bin=float("inf")), "t_bin must be finite and at least 0"),
    (dict(frames=2, t_bin=0.0), "a steady map \\(t_bin == 0\\) has one frame"),
    (dict(t_min=float("inf")), "t_min must be finite"),
    (dict(cos_min=1.0), "cos_min must lie in 0 <= cos_min < 1"),
    (dict(cos_min=-0.1), "cos_min must lie in 0 <= cos_min < 1"),
    (dict(cos_min=float("nan")), "cos_min must lie in 0 <= cos_min < 1"),
    (dict(reserved=1), "reserved must be 0"),
    (dict(res=(4096, 4096), frames=2, t_bin=0.5), "more than 2\\^27 cells x faces x frames"),
    (dict(boundary=P.BOUNDARY_SPHERE, res=(4096, 4096), frames=9, t_bin=0.5), "more than 2\\^27 cells x faces x frames"),
])
def test_validate_exitance_refuses(kw, msg):
    with pytest.raises(capi.MerError, match="^mer_exitance_create: .*" + msg):
        capi.validate_exitance(_desc(**kw))


def test_validate_exitance_accepts():
    capi.validate_exitance(_desc())
    capi.validate_exitance(_desc(boundary=P.BOUNDARY_SPHERE, res=(1, 1), frames=4096, t_min=-3.0, t_bin=1e-3, cos_min=0.999))
    capi.validate_exitance(_desc(boundary=P.BOUNDARY_SPHERE, res=(4096, 4096), frames=8, t_bin=0.5))       # exactly 2^27 keys
    capi.validate_exitance(_desc(res=(2048, 2048), frames=5, t_bin=0.5))                                   # 6 faces: 1.26e8 < 2^27
    assert capi.exitance_faces(P.BOUNDARY_AABB) == 6 and capi.exitance_faces(P.BOUNDARY_SPHERE) == 1


def _run(*args):
    r = subprocess.run([MER_RENDER, *args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


@pytest.mark.parametrize("args,msg", [
    (["--exitance=8,8", "--fluence=8,8,8"], "--exitance and --fluence exclude each other"),
    (["--exitance=8,8", "--gpus", "2"], "--exitance runs on one GPU"),
    (["--exitance=8,8", "--devices", "0,0"], "--exitance runs on one GPU"),
    (["--exitance=8,8", "--track-length"], "--track-length belongs to --fluence"),
    (["--exitance=8,8", "-o", "exit.vol"], "--exitance writes a .npy file"),
    (["--exitance=8,8", "--time-resolved", "-o", "exit.pfm"], "--exitance writes a .npy file"),
    (["--exitance=8"], "--exitance=NU,NV expects two cell counts"),
    (["--exitance=8,0"], "--exitance=NU,NV expects two cell counts"),
    (["--exitance=8,4097"], "--exitance=NU,NV expects two cell counts"),
    (["--exitance=8,8,8"], "--exitance=NU,NV expects two cell counts"),
    (["--exitance"], "--exitance=NU,NV expects two cell counts"),
    (["--exitance=8,8", "--accept-cos=1"], "--accept-cos=C expects a cosine with 0 <= C < 1"),
    (["--exitance=8,8", "--accept-cos=x"], "--accept-cos=C expects a cosine with 0 <= C < 1"),
    (["--accept-cos=0.5"], "--accept-cos needs --exitance=NU,NV"),
])
def test_mer_render_refuses(args, msg):
    rc, err = _run(*args, SCENE)
    assert rc == 2 and msg in err, (rc, err)
    for name in ("exit.vol", "exit.pfm"):
        assert not os.path.exists(name)


def test_mer_render_keeps_the_messages_of_fluence():
    rc, err = _run("--time-resolved", SCENE)
    assert rc == 2 and "--time-resolved needs --fluence=NX,NY,NZ" in err, (rc, err)
    rc, err = _run("--fluence=8,8,8", "--gpus", "2", SCENE)
    assert rc == 2 and "--fluence runs on one GPU" in err, (rc, err)


def test_mer_render_refuses_time_resolved_without_a_transient_film(tmp_path):
    """the window comes from the film: the laser scene with decomposition = none is refused by name, before any device is touched"""
    xml = open(SCENE).read()
    scene = tmp_path / "laser_steady.xml"
    scene.write_text(xml.replace('<string name="decomposition" value="transient"/>', '<string name="decomposition" value="none"/>'))
    rc, err = _run("--exitance=8,8", "--time-resolved", "-o", str(tmp_path / "exit.npy"), "-D", "samples=2", "-D", "tMin=4", "-D", "tMax=9", "-D", "tRes=0.5",
                   "-D", "medium=homogeneous", str(scene))
    assert rc == 1 and "decomposition = transient" in err, (rc, err)
    assert not (tmp_path / "exit.npy").exists()
