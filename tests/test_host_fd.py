"""The frequency-domain recorders' interface without a GPU: the header declares the four entry points and both libraries export them, the
ctypes mirrors of mer_fluence_fd_desc and mer_exitance_fd_desc have the C compiler's size and offsets (and no implicit padding), the ABI
version and mer_scene_desc are untouched, validate_fluence_fd / validate_exitance_fd refuse what the create entry points refuse, with their
messages, and `mer_render --frequencies` refuses by name what it is not built for while it still parses its arguments."""
import ctypes
import os
import re
import subprocess
import tempfile
import pytest
from mitsubaer_amd import capi, params as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ["mer_fluence_fd_create", "mer_fluence_fd_read", "mer_exitance_fd_create", "mer_exitance_fd_read"]
MER_RENDER = os.path.join(ROOT, "mitsubaer_amd", "mer_render")
SCENE = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
BOX = ((4, 4, 4), (-1, -1, -1), (1, 1, 1))


def test_header_declares_and_libraries_export_the_entry_points():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mer.h")).read(), flags=re.S)
    for f in FUNCTIONS:
        assert re.search(r"\bint\s+%s\s*\(" % f, txt), f
        assert f in capi.SYMBOLS
        assert hasattr(capi.lib(), f) and hasattr(capi.lib(capi.CHECK_LIB_PATH), f), f
    assert "MER_ABI_VERSION 3" in txt and re.search(r"#define\s+MER_MAX_FREQUENCIES\s+8\b", txt)
    assert capi.MAX_FREQUENCIES == 8


def _layout(struct, fields):
    src = ('#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%%zu", sizeof(%s));\n' % struct
           + "".join('printf(" %%zu", offsetof(%s, %s));\n' % (struct, f) for f in fields) + 'printf(" %zu %d\\n", sizeof(mer_scene_desc), MER_ABI_VERSION);return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        size, *rest = map(int, subprocess.check_output([os.path.join(d, "t")]).split())
    return size, rest[:-2], rest[-2], rest[-1]


def test_desc_mirrors_have_the_compilers_size_and_offsets():
    fields = ["res", "bmin", "bmax", "n_freq", "reserved", "wavenumber"]
    size, offsets, scene, abi = _layout("mer_fluence_fd_desc", fields)
    assert ctypes.sizeof(capi.FluenceFDDesc) == size == 48 + 64               # the sum of the fields: no implicit padding
    assert [getattr(capi.FluenceFDDesc, f).offset for f in fields] == offsets == [0, 12, 24, 36, 40, 48]
    assert scene == ctypes.sizeof(capi.SceneDesc) and abi == 3
    fields = ["boundary", "res", "cos_min", "n_freq", "reserved", "wavenumber"]
    size, offsets, scene, abi = _layout("mer_exitance_fd_desc", fields)
    assert ctypes.sizeof(capi.ExitanceFDDesc) == size == 24 + 64
    assert [getattr(capi.ExitanceFDDesc, f).offset for f in fields] == offsets == [0, 4, 12, 16, 20, 24]
    assert scene == ctypes.sizeof(capi.SceneDesc) and abi == 3


def test_the_scene_desc_is_unchanged():
    """sizeof(mer_scene_desc) of ABI version 3, as the header gave it before these recorders (tests/test_abi.py compares the mirror with
    the compiler; this pins the number)"""
    assert _layout("mer_fluence_fd_desc", ["res"])[2] == ctypes.sizeof(capi.SceneDesc) == 472


def _grid(res=BOX[0], bmin=BOX[1], bmax=BOX[2], k=(0.0, 0.7), reserved=(0, 0), tail=None, n_freq=None):
    d = capi.fluence_fd_desc(res, bmin, bmax, k)
    d.reserved[:] = reserved
    if tail is not None:
        d.wavenumber[7] = tail
    if n_freq is not None:
        d.n_freq = n_freq
    return d


def _map(boundary=P.BOUNDARY_AABB, res=(4, 4), k=(0.0, 0.7), cos_min=0.0, reserved=0, tail=None, n_freq=None):
    d = capi.exitance_fd_desc(boundary, res, k, cos_min)
    d.reserved = reserved
    if tail is not None:
        d.wavenumber[7] = tail
    if n_freq is not None:
        d.n_freq = n_freq
    return d


FREQ_REFUSALS = [
    (dict(k=()), "n_freq must lie in 1 ... 8"),
    (dict(k=(0.1,) * 9), "n_freq must lie in 1 ... 8"),
    (dict(n_freq=-1), "n_freq must lie in 1 ... 8"),
    (dict(k=(0.5, -0.1)), "a wavenumber must be finite and at least 0"),
    (dict(k=(float("nan"),)), "a wavenumber must be finite and at least 0"),
    (dict(k=(1.0, float("inf"))), "a wavenumber must be finite and at least 0"),
    (dict(tail=0.3), "the entries of wavenumber past n_freq must be 0"),
    (dict(tail=float("nan")), "the entries of wavenumber past n_freq must be 0"),
]


@pytest.mark.parametrize("kw,msg", FREQ_REFUSALS + [
    (dict(res=(0, 4, 4)), "res must lie in 1 ... 1024 on every axis"),
    (dict(bmin=(-1, float("nan"), -1)), "bmin / bmax must be finite"),
    (dict(bmin=(1, -1, -1)), "bmin must be below bmax on every axis"),
    (dict(res=(1024, 1024, 1024)), "more than 2\\^27 cells"),
    (dict(reserved=(1, 0)), "reserved must be 0"),
    (dict(reserved=(0, 1)), "reserved must be 0"),
    (dict(res=(512, 512, 512), k=(0.5,)), "more than 2\\^27 cells x 2 x n_freq"),
    (dict(res=(256, 256, 256), k=(0.5,) * 8), "more than 2\\^27 cells x 2 x n_freq"),
])
def test_validate_fluence_fd_refuses(kw, msg):
    with pytest.raises(capi.MerError, match="^mer_fluence_fd_create: " + msg):
        capi.validate_fluence_fd(_grid(**kw))


@pytest.mark.parametrize("kw,msg", FREQ_REFUSALS + [
    (dict(boundary=P.BOUNDARY_SDF), "boundary must be the cube .* or the sphere"),
    (dict(res=(0, 8)), "res must lie in 1 ... 4096"),
    (dict(cos_min=1.0), "cos_min must lie in 0 <= cos_min < 1"),
    (dict(cos_min=float("nan")), "cos_min must lie in 0 <= cos_min < 1"),
    (dict(reserved=1), "reserved must be 0"),
    (dict(res=(4096, 4096), k=(0.5,)), "more than 2\\^27 cells x faces x 2 x n_freq"),
    (dict(boundary=P.BOUNDARY_SPHERE, res=(4096, 4096), k=(0.5,) * 5), "more than 2\\^27 cells x faces x 2 x n_freq"),
])
def test_validate_exitance_fd_refuses(kw, msg):
    with pytest.raises(capi.MerError, match="^mer_exitance_fd_create: " + msg):
        capi.validate_exitance_fd(_map(**kw))


def test_validators_accept():
    capi.validate_fluence_fd(_grid())
    capi.validate_fluence_fd(_grid(k=(0.0,)))
    capi.validate_fluence_fd(_grid(res=(128, 128, 128), k=tuple(range(8))))                   # 2^21 x 16 = 2^25
    capi.validate_fluence_fd(_grid(res=(256, 256, 256), k=(1.0, 2.0, 3.0, 4.0)))              # exactly 2^27 keys
    capi.validate_exitance_fd(_map())
    capi.validate_exitance_fd(_map(boundary=P.BOUNDARY_SPHERE, res=(4096, 4096), k=(0.5,) * 4, cos_min=0.999))     # exactly 2^27 keys
    d = _grid(k=(0.0, 0.7, 3.0))
    assert d.n_freq == 3 and list(d.wavenumber) == [0.0, 0.7, 3.0, 0, 0, 0, 0, 0]
    for name in ("fluence_fd_create", "fluence_fd_read", "exitance_fd_create", "exitance_fd_read"):
        assert callable(getattr(capi.Context, name))


def _run(*args):
    r = subprocess.run([MER_RENDER, *args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


@pytest.mark.parametrize("args,msg", [
    (["--frequencies=0,0.7"], "--frequencies needs --fluence=NX,NY,NZ or --exitance=NU,NV"),
    (["--fluence=4,4,4", "--frequencies=0.7", "--time-resolved"], "--frequencies and --time-resolved exclude each other"),
    (["--exitance=4,4", "--frequencies=0.7", "--time-resolved"], "--frequencies and --time-resolved exclude each other"),
    (["--fluence=4,4,4", "--frequencies=0.7", "--track-length"], "--frequencies and --track-length exclude each other"),
    (["--sensitivity=4,4,4", "--detector=5,4,4,0,4,0,4", "--frequencies=0.7"], "--frequencies belongs to --fluence / --exitance"),
    (["--fluence=4,4,4", "--frequencies=0.7", "--gpus", "2"], "--frequencies runs on one GPU"),
    (["--exitance=4,4", "--frequencies=0.7", "--devices", "0,0"], "--frequencies runs on one GPU"),
    (["--fluence=4,4,4", "--frequencies"], "--frequencies=K1[,K2,...] expects a comma-separated list of wavenumbers"),
    (["--fluence=4,4,4", "--frequencies="], "--frequencies=K1[,K2,...] expects a comma-separated list of wavenumbers"),
    (["--fluence=4,4,4", "--frequencies=0.7,"], "--frequencies=K1[,K2,...] expects a comma-separated list of wavenumbers"),
    (["--fluence=4,4,4", "--frequencies=0.7,,1"], "--frequencies=K1[,K2,...] expects a comma-separated list of wavenumbers"),
    (["--fluence=4,4,4", "--frequencies=0.7;1"], "--frequencies=K1[,K2,...] expects a comma-separated list of wavenumbers"),
    (["--exitance=4,4", "--frequencies=1x"], "--frequencies=K1[,K2,...] expects a comma-separated list of wavenumbers"),
    (["--fluence=4,4,4", "--frequencies=1,2,3,4,5,6,7,8,9"], "--frequencies takes at most 8 wavenumbers"),
    (["--fluence=4,4,4", "--frequencies=0.7,-1"], "--frequencies: a wavenumber must be finite and at least 0"),
    (["--exitance=4,4", "--frequencies=inf"], "--frequencies: a wavenumber must be finite and at least 0"),
    (["--exitance=4,4", "--frequencies=nan"], "--frequencies: a wavenumber must be finite and at least 0"),
    (["--fluence=4,4,4", "--frequencies=0.7", "-o", "fd.vol"], "--frequencies writes a .npy file"),
    (["--exitance=4,4", "--frequencies=0.7", "-o", "fd.pfm"], "--exitance writes a .npy file"),
])
def test_mer_render_refuses(args, msg):
    rc, err = _run(*args, SCENE)
    assert rc == 2 and msg in err, (rc, err)
    for name in ("fd.vol", "fd.pfm"):
        assert not os.path.exists(name)


def test_mer_render_keeps_the_messages_of_its_neighbours():
    rc, err = _run("--exitance=8,8", "--fluence=8,8,8", "--frequencies=1", SCENE)
    assert rc == 2 and "--exitance and --fluence exclude each other" in err, (rc, err)
    rc, err = _run("--time-resolved", SCENE)
    assert rc == 2 and "--time-resolved needs --fluence=NX,NY,NZ" in err, (rc, err)
    rc, err = _run("--accept-cos=0.5", "--fluence=4,4,4", "--frequencies=1", SCENE)
    assert rc == 2 and "--accept-cos needs --exitance=NU,NV" in err, (rc, err)
