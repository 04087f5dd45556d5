"""The interface of the detector arrays of the sensitivity grid without a GPU: the header declares the three entry points and both
libraries export them, the ctypes mirror of mer_sensitivity_array_desc has the C compiler's size and offsets, validate_sensitivity_array
refuses what mer_sensitivity_array_create refuses, with its messages, and `mer_render` refuses --detector-bins, --gates and --scatter by
name where they do not belong, while it still parses its arguments."""
import ctypes
import os
import re
import subprocess
import tempfile
import pytest
from mitsubaer_amd import capi, params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["mer_sensitivity_array_create", "mer_sensitivity_shape", "mer_sensitivity_read_array"]
MER_RENDER = os.path.join(ROOT, "mitsubaer_amd", "mer_render")
SCENE = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
DET = "--detector=5,4,4,0,4,0,4"
SENS = "--sensitivity=8,8,8"


def test_header_declares_and_libraries_export_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mer.h")).read(), flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % f, txt), f
        assert f in capi.SYMBOLS
        assert hasattr(capi.lib(), f) and hasattr(capi.lib(capi.CHECK_LIB_PATH), f), f
    assert txt.index("mer_sensitivity_desc;") < txt.index("mer_sensitivity_array_desc;") < txt.index("mer_sensitivity_array_create")
    assert "MER_ABI_VERSION 3" in txt                                        # the ABI only grew


def test_desc_mirror_has_the_compilers_size_and_offsets():
    fields = ["res", "bmin", "bmax", "det", "bin_u", "bin_v", "gates", "scatter", "reserved"]
    src = ('#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu", sizeof(mer_sensitivity_array_desc));\n'
           + "".join('printf(" %%zu", offsetof(mer_sensitivity_array_desc, %s));\n' % f for f in fields) + 'printf("\\n");return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        got = list(map(int, subprocess.check_output([os.path.join(d, "t")]).split()))
    assert ctypes.sizeof(capi.SensitivityArrayDesc) == got[0] == 108
    assert [getattr(capi.SensitivityArrayDesc, f).offset for f in fields] == got[1:] == [0, 12, 24, 36, 84, 88, 92, 96, 100]


def _desc(res=(8, 8, 8), bmin=(-1, -1, -1), bmax=(1, 1, 1), boundary=P.BOUNDARY_AABB, dres=(8, 8), face=5, window=(2, 6, 2, 6), cos_min=0.0, t_min=0.0,
          t_bin=0.0, det_reserved=0, bins=(2, 2), gates=1, scatter=0, reserved=(0, 0)):
    det = capi.detector_desc(boundary, dres, face, window, cos_min, t_min, t_bin)
    det.reserved = det_reserved
    d = capi.sensitivity_array_desc(res, bmin, bmax, det, bins, gates)
    d.scatter = scatter
    d.reserved[:] = reserved
    return d


@pytest.mark.parametrize("kw,msg", [
    # what mer_sensitivity_create refuses, in its words
    (dict(res=(0, 8, 8)), "res must lie in 1 ... 1024 on every axis"),
    (dict(bmax=(1, 1, float("inf"))), "bmin / bmax must be finite"),
    (dict(bmin=(-1, 1, -1)), "bmin must be below bmax on every axis"),
    (dict(res=(1024, 1024, 256)), "more than 2\\^27 cells"),
    (dict(boundary=P.BOUNDARY_SDF), "boundary must be the cube .* or the sphere"),
    (dict(dres=(0, 8)), "detector res must lie in 1 ... 4096"),
    (dict(t_bin=-0.5), "t_bin must be finite and at least 0"),
    (dict(t_min=float("inf")), "t_min must be finite"),
    (dict(cos_min=1.0), "cos_min must lie in 0 <= cos_min < 1"),
    (dict(det_reserved=1), "reserved must be 0"),
    (dict(face=6), "face must be one of the boundary's faces"),
    (dict(window=(0, 9, 0, 4)), "the window must lie inside the raster"),
    (dict(window=(4, 4, 0, 4)), "the window is empty"),
    # its own
    (dict(bins=(0, 2)), "bin_u and bin_v must be at least 1"),
    (dict(bins=(2, -1)), "bin_u and bin_v must be at least 1"),
    (dict(bins=(3, 2)), "bin_u and bin_v must divide the window"),
    (dict(bins=(2, 8)), "bin_u and bin_v must divide the window"),
    (dict(gates=0), "gates must be at least 1"),
    (dict(gates=2), "several gates need t_bin > 0"),
    (dict(scatter=2), "scatter must be 0 or 1"),
    (dict(scatter=-1), "scatter must be 0 or 1"),
    (dict(reserved=(0, 1)), "reserved must be 0"),
    (dict(reserved=(1, 0)), "reserved must be 0"),
    (dict(res=(512, 512, 256), bins=(2, 2)), "more than 2\\^27 cells x measurements x \\(1 \\+ scatter\\)"),
    (dict(res=(512, 512, 256), bins=(4, 2), scatter=1), "more than 2\\^27 cells x measurements x \\(1 \\+ scatter\\)"),
    (dict(res=(64, 64, 64), bins=(4, 4), gates=513, t_bin=0.1), "more than 2\\^27 cells x measurements x \\(1 \\+ scatter\\)"),
])
def test_validate_sensitivity_array_refuses(kw, msg):
    with pytest.raises(capi.MerError, match="^mer_sensitivity_array_create: .*" + msg):
        capi.validate_sensitivity_array(_desc(**kw))


def test_validate_sensitivity_array_accepts():
    capi.validate_sensitivity_array(_desc())
    capi.validate_sensitivity_array(_desc(bins=(1, 1), gates=8, t_bin=0.25, scatter=1))
    capi.validate_sensitivity_array(_desc(res=(512, 512, 256), bins=(4, 4), scatter=1, gates=1))             # exactly 2^27 keys
    capi.validate_sensitivity_array(_desc(res=(64, 64, 64), bins=(4, 4), gates=512, t_bin=0.1))
    d = capi.sensitivity_array_desc((4, 4, 4), (-1, -1, -1), (1, 1, 1), capi.detector_desc(P.BOUNDARY_AABB, (6, 3), 2), None)      # no bins: one detector
    assert (d.bin_u, d.bin_v, d.gates, d.scatter) == (6, 3, 1, 0)
    assert capi.sensitivity_array_shape(_desc(bins=(2, 1), gates=3, t_bin=1.0, scatter=1)) == (2, 3, 4, 2)
    assert capi.SENSITIVITY_ARRAY_TOTALS[:7] == capi.SENSITIVITY_TOTALS and len(capi.SENSITIVITY_ARRAY_TOTALS) == 8


def _run(*args):
    r = subprocess.run([MER_RENDER, *args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


NEEDS = "--detector-bins, --gates and --scatter need --sensitivity=NX,NY,NZ and --detector=FACE,NU,NV,IU0,IU1,IV0,IV1"


@pytest.mark.parametrize("args,msg", [
    (["--scatter"], NEEDS),
    (["--gates=2"], NEEDS),
    (["--detector-bins=2,2"], NEEDS),
    (["--fluence=8,8,8", "--scatter"], NEEDS),
    (["--exitance=4,4", "--detector-bins=2,2"], NEEDS),
    ([SENS, "--scatter"], "--sensitivity needs --detector="),
    ([SENS, DET, "--gates=2"], "--gates=N above 1 needs --gate=TMIN,TBIN"),
    ([SENS, DET, "--gates=0"], "--gates=N expects a count of at least 1"),
    ([SENS, DET, "--gates=x"], "--gates=N expects a count of at least 1"),
    ([SENS, DET, "--detector-bins=2"], "--detector-bins=BU,BV expects two cell counts"),
    ([SENS, DET, "--detector-bins=0,2"], "--detector-bins=BU,BV expects two cell counts"),
    ([SENS, DET, "--detector-bins=3,2"], "--detector-bins=BU,BV must divide the window"),
    ([SENS, DET, "--scatter", "-o", "k.vol"], "write a .npy file"),
    # without them the command is as it was
    ([SENS, DET, "--time-resolved"], "a sensitivity grid has the one gate of --gate=TMIN,TBIN"),
    ([SENS, DET, "--scatter", "--time-resolved"], "a sensitivity grid has the one gate of --gate=TMIN,TBIN"),
    ([SENS, DET, "--scatter", "--gpus", "2"], "--sensitivity runs on one GPU"),
])
def test_mer_render_refuses(args, msg):
    rc, err = _run(*args, SCENE)
    assert rc == 2 and msg in err, (rc, err)
    assert not os.path.exists("sensitivity.npy") and not os.path.exists("sensitivity.vol")


def test_mer_render_usage_names_the_options():
    r = subprocess.run([MER_RENDER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "[--gate=TMIN,TBIN] [--detector-bins=BU,BV] [--gates=N] [--scatter]] scene.xml" in r.stdout
    assert "--detector-bins=BU,BV, --gates=N, --scatter (with --sensitivity= and --detector=)" in r.stdout
