"""The sensitivity grid's interface without a GPU: the header declares the five entry points and both libraries export them, the ctypes
mirrors of mer_detector_desc and mer_sensitivity_desc have the C compiler's size and offsets, validate_sensitivity refuses what
mer_sensitivity_create refuses, with its messages, and `mer_render --sensitivity` refuses by name what it is not built for while it still
parses its arguments."""
import ctypes
import os
import re
import subprocess
import tempfile
import pytest
from mitsubaer_amd import capi, params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["mer_sensitivity_create", "mer_sensitivity_clear", "mer_sensitivity_destroy", "mer_render_sensitivity", "mer_sensitivity_read"]
MER_RENDER = os.path.join(ROOT, "mitsubaer_amd", "mer_render")
SCENE = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
DET = "--detector=5,4,4,1,3,1,3"


def test_header_declares_and_libraries_export_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mer.h")).read(), flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % f, txt), f
        assert f in capi.SYMBOLS
        assert hasattr(capi.lib(), f) and hasattr(capi.lib(capi.CHECK_LIB_PATH), f), f
    assert txt.index("} mer_shard;") < txt.index("mer_detector_desc;") < txt.index("mer_sensitivity_desc;") < txt.index("mer_sensitivity_create")
    assert "MER_ABI_VERSION 3" in txt


def test_desc_mirrors_have_the_compilers_size_and_offsets():
    det = ["boundary", "res", "face", "iu0", "iu1", "iv0", "iv1", "cos_min", "t_min", "t_bin", "reserved"]
    sens = ["res", "bmin", "bmax", "det"]
    src = ('#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(mer_detector_desc));\n'
           + "".join('printf(" %%zu", offsetof(mer_detector_desc, %s));\n' % f for f in det) + 'printf(" %zu", sizeof(mer_sensitivity_desc));\n'
           + "".join('printf(" %%zu", offsetof(mer_sensitivity_desc, %s));\n' % f for f in sens) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    assert ctypes.sizeof(capi.DetectorDesc) == got[0] == 48
    assert [getattr(capi.DetectorDesc, f).offset for f in det] == got[1:12] == [0, 4, 12, 16, 20, 24, 28, 32, 36, 40, 44]
    assert ctypes.sizeof(capi.SensitivityDesc) == got[12] == 84
    assert [getattr(capi.SensitivityDesc, f).offset for f in sens] == got[13:] == [0, 12, 24, 36]


def _desc(res=(8, 8, 8), bmin=(-1, -1, -1), bmax=(1, 1, 1), boundary=P.BOUNDARY_AABB, dres=(8, 8), face=5, window=(2, 6, 2, 6), cos_min=0.0, t_min=0.0,
          t_bin=0.0, reserved=0):
    det = capi.detector_desc(boundary, dres, face, window, cos_min, t_min, t_bin)
    det.reserved = reserved
    return capi.sensitivity_desc(res, bmin, bmax, det)


@pytest.mark.parametrize("kw,msg", [
    (dict(res=(0, 8, 8)), "res must lie in 1 ... 1024 on every axis"),
    (dict(res=(8, 8, 1025)), "res must lie in 1 ... 1024 on every axis"),
    (dict(bmin=(-1, float("nan"), -1)), "bmin / bmax must be finite"),
    (dict(bmax=(1, 1, float("inf"))), "bmin / bmax must be finite"),
    (dict(bmin=(-1, 1, -1)), "bmin must be below bmax on every axis"),
    (dict(res=(1024, 1024, 256)), "more than 2\\^27 cells"),
    (dict(boundary=P.BOUNDARY_SDF), "boundary must be the cube .* or the sphere"),
    (dict(dres=(0, 8)), "detector res must lie in 1 ... 4096"),
    (dict(dres=(8, 4097), window=(0, 1, 0, 1)), "detector res must lie in 1 ... 4096"),
    (dict(t_bin=-0.5), "t_bin must be finite and at least 0"),
    (dict(t_bin=float("nan")), "t_bin must be finite and at least 0"),
    (dict(t_bin=float("inf")), "t_bin must be finite and at least 0"),
    (dict(t_min=float("inf")), "t_min must be finite"),
    (dict(cos_min=1.0), "cos_min must lie in 0 <= cos_min < 1"),
    (dict(cos_min=-0.1), "cos_min must lie in 0 <= cos_min < 1"),
    (dict(cos_min=float("nan")), "cos_min must lie in 0 <= cos_min < 1"),
    (dict(reserved=1), "reserved must be 0"),
    (dict(face=6), "face must be one of the boundary's faces"),
    (dict(face=-1), "face must be one of the boundary's faces"),
    (dict(boundary=P.BOUNDARY_SPHERE, face=1), "face must be one of the boundary's faces"),
    (dict(window=(-1, 4, 0, 4)), "the window must lie inside the raster"),
    (dict(window=(0, 9, 0, 4)), "the window must lie inside the raster"),
    (dict(window=(0, 4, 0, 9)), "the window must lie inside the raster"),
    (dict(window=(0, 4, -2, 4)), "the window must lie inside the raster"),
    (dict(window=(4, 4, 0, 4)), "the window is empty"),
    (dict(window=(0, 4, 5, 3)), "the window is empty"),
])
def test_validate_sensitivity_refuses(kw, msg):
    with pytest.raises(capi.MerError, match="^mer_sensitivity_create: .*" + msg):
        capi.validate_sensitivity(_desc(**kw))


def test_validate_sensitivity_accepts():
    capi.validate_sensitivity(_desc())
    capi.validate_sensitivity(_desc(res=(1024, 1024, 128), boundary=P.BOUNDARY_SPHERE, dres=(4096, 1), face=0, window=(0, 4096, 0, 1), cos_min=0.999,
                                    t_min=-3.0, t_bin=1e-3))
    d = capi.detector_desc(P.BOUNDARY_AABB, (6, 3), 2)                         # no window: the whole face
    assert (d.iu0, d.iu1, d.iv0, d.iv1) == (0, 6, 0, 3)
    assert capi.SENSITIVITY_TOTALS[0] == "paths" and len(capi.SENSITIVITY_TOTALS) == 7


def _run(*args):
    r = subprocess.run([MER_RENDER, *args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


@pytest.mark.parametrize("args,msg", [
    (["--sensitivity=8,8,8", DET, "--fluence=8,8,8"], "--sensitivity excludes --fluence and --exitance"),
    (["--sensitivity=8,8,8", DET, "--exitance=8,8"], "--sensitivity excludes --fluence and --exitance"),
    (["--sensitivity=8,8,8", DET, "--gpus", "2"], "--sensitivity runs on one GPU"),
    (["--sensitivity=8,8,8", DET, "--devices", "0,0"], "--sensitivity runs on one GPU"),
    (["--sensitivity=8,8,8", DET, "--time-resolved"], "a sensitivity grid has the one gate of --gate=TMIN,TBIN"),
    (["--sensitivity=8,8,8", DET, "--track-length"], "a sensitivity grid has the one gate of --gate=TMIN,TBIN"),
    (["--sensitivity=8,8,8"], "--sensitivity needs --detector=FACE,NU,NV,IU0,IU1,IV0,IV1"),
    (["--sensitivity=8,8"], "--sensitivity=NX,NY,NZ expects three cell counts"),
    (["--sensitivity=8,8,0"], "--sensitivity=NX,NY,NZ expects three cell counts"),
    (["--sensitivity=8,8,1025"], "--sensitivity=NX,NY,NZ expects three cell counts"),
    (["--sensitivity"], "--sensitivity=NX,NY,NZ expects three cell counts"),
    (["--sensitivity=8,8,8", "--detector=6,4,4,0,4,0,4"], "--detector=FACE,NU,NV,IU0,IU1,IV0,IV1 expects"),
    (["--sensitivity=8,8,8", "--detector=5,4,4,0,5,0,4"], "--detector=FACE,NU,NV,IU0,IU1,IV0,IV1 expects"),
    (["--sensitivity=8,8,8", "--detector=5,4,4,2,2,0,4"], "--detector=FACE,NU,NV,IU0,IU1,IV0,IV1 expects"),
    (["--sensitivity=8,8,8", "--detector=5,4,4,0,4"], "--detector=FACE,NU,NV,IU0,IU1,IV0,IV1 expects"),
    (["--sensitivity=8,8,8", "--detector=5,0,4,0,4,0,4"], "--detector=FACE,NU,NV,IU0,IU1,IV0,IV1 expects"),
    (["--sensitivity=8,8,8", DET, "--gate=2"], "--gate=TMIN,TBIN expects"),
    (["--sensitivity=8,8,8", DET, "--gate=2,0"], "--gate=TMIN,TBIN expects"),
    (["--sensitivity=8,8,8", DET, "--gate=2,x"], "--gate=TMIN,TBIN expects"),
    (["--sensitivity=8,8,8", DET, "--accept-cos=1"], "--accept-cos=C expects a cosine with 0 <= C < 1"),
    ([DET], "--detector and --gate need --sensitivity=NX,NY,NZ"),
    (["--gate=2,1"], "--detector and --gate need --sensitivity=NX,NY,NZ"),
    (["--fluence=8,8,8", DET], "--detector and --gate need --sensitivity=NX,NY,NZ"),
])
def test_mer_render_refuses(args, msg):
    rc, err = _run(*args, SCENE)
    assert rc == 2 and msg in err, (rc, err)
    assert not os.path.exists("sensitivity.vol")


def test_mer_render_usage_names_the_option_and_what_it_excludes():
    r = subprocess.run([MER_RENDER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "--sensitivity=NX,NY,NZ --detector=FACE,NU,NV,IU0,IU1,IV0,IV1 [--accept-cos=C] [--gate=TMIN,TBIN]" in r.stdout
    assert "not with --fluence, --exitance, --gpus or --devices" in r.stdout


# the box checks are one helper under the caller's prefix: each composed form says its own entry point's name, once, and no other's
BOX_REFUSALS = [(dict(res=(0, 8, 8)), "res must lie in 1 ... 1024 on every axis"), (dict(bmin=(-1, float("nan"), -1)), "bmin / bmax must be finite"),
                (dict(bmin=(-1, 1, -1)), "bmin must be below bmax on every axis"), (dict(res=(1024, 1024, 256)), "more than 2^27 cells")]
COMPOSED = {
    "mer_fluence_create": lambda res, bmin, bmax: capi.validate_fluence(capi.fluence_desc(res, bmin, bmax)),
    "mer_fluence_track_create": lambda res, bmin, bmax: capi.validate_fluence_track(capi.fluence_desc(res, bmin, bmax)),
    "mer_fluence_time_create": lambda res, bmin, bmax: capi.validate_fluence_time(capi.fluence_time_desc(res, bmin, bmax, 4, 0.0, 1.0)),
    "mer_sensitivity_create": lambda res, bmin, bmax: capi.validate_sensitivity(_desc(res=res, bmin=bmin, bmax=bmax)),
}


@pytest.mark.parametrize("who", sorted(COMPOSED))
@pytest.mark.parametrize("kw,msg", BOX_REFUSALS)
def test_box_refusals_carry_their_own_prefix_once(who, kw, msg):
    box = dict(res=(8, 8, 8), bmin=(-1, -1, -1), bmax=(1, 1, 1))
    COMPOSED[who](**box)                                # accepted as it stands
    box.update(kw)
    with pytest.raises(capi.MerError) as e:
        COMPOSED[who](**box)
    assert str(e.value) == who + ": " + msg
    assert len(re.findall(r"mer_\w+_create", str(e.value))) == 1


def test_raster_refusals_carry_their_own_prefix_once():
    """the raster / gate / cone checks are shared the same way between the exitance map and the detector"""
    for make, who, res_what in ((lambda **kw: capi.validate_exitance(capi.exitance_desc(kw.pop("boundary", P.BOUNDARY_AABB), kw.pop("dres", (8, 8)), **kw)),
                                 "mer_exitance_create", "res"),
                                (lambda **kw: capi.validate_sensitivity(_desc(**kw)), "mer_sensitivity_create", "detector res")):
        for kw, msg in ((dict(boundary=P.BOUNDARY_SDF), "boundary must be the cube (MER_BOUNDARY_AABB) or the sphere (MER_BOUNDARY_SPHERE)"),
                        (dict(dres=(0, 8)), res_what + " must lie in 1 ... 4096 on both axes"), (dict(t_bin=-0.5), "t_bin must be finite and at least 0"),
                        (dict(t_min=float("inf")), "t_min must be finite"), (dict(cos_min=1.0), "cos_min must lie in 0 <= cos_min < 1")):
            with pytest.raises(capi.MerError) as e:
                make(**kw)
            assert str(e.value) == who + ": " + msg
