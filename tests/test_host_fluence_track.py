"""The track-length fluence grid's interface without a GPU: the header declares mer_fluence_track_create and both libraries export it, the
ABI version is unchanged, and `mer_render` refuses --track-length without --fluence= and together with --time-resolved while it still parses
its arguments (exit status 2, no scene read, no device touched)."""
import os
import re
import subprocess
import pytest
from mitsubaer_amd import capi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MER_RENDER = os.path.join(ROOT, "mitsubaer_amd", "mer_render")
SCENE = os.path.join(ROOT, "scenes", "cfg_laser_clear.xml")


def test_header_declares_and_libraries_export_the_entry_point():
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mer.h")).read(), flags=re.S)
    f = "mer_fluence_track_create"
    assert re.search(r"\bint\s+%s\s*\(\s*mer_context\s*\*\s*\w*\s*,\s*const\s+mer_fluence_desc\s*\*\s*\w*\s*,\s*mer_fluence\s*\*\s*\w*\s*\)" % f, txt)
    assert f in capi.SYMBOLS
    assert hasattr(capi.lib(), f) and hasattr(capi.lib(capi.CHECK_LIB_PATH), f)
    assert "MER_ABI_VERSION 3" in txt


def test_python_front_end_knows_the_estimator():
    assert hasattr(capi.Context, "fluence_track_create")
    import inspect
    assert inspect.signature(capi.Context.fluence).parameters["estimator"].default == "collision"


def _run(*args):
    r = subprocess.run([MER_RENDER, *args], capture_output=True, text=True, timeout=60)
    return r.returncode, r.stderr


@pytest.mark.parametrize("args", [["--track-length"], ["--track-length", "-D", "samples=2"], ["-s", "2", "--track-length"]])
def test_mer_render_refuses_track_length_without_fluence(args):
    rc, err = _run(*args, SCENE)
    assert rc == 2 and "--track-length needs --fluence=NX,NY,NZ" in err, (rc, err)


@pytest.mark.parametrize("args", [["--fluence=8,8,8", "--track-length", "--time-resolved"], ["--time-resolved", "--track-length", "--fluence=8,8,8"]])
def test_mer_render_refuses_track_length_with_time_resolved(args):
    rc, err = _run(*args, SCENE)
    assert rc == 2 and "--track-length and --time-resolved exclude each other" in err, (rc, err)


def test_usage_names_the_option():
    r = subprocess.run([MER_RENDER, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0 and "--track-length" in r.stdout


def test_example_scene_is_grey_analog_and_clear_on_demand():
    """scenes/cfg_laser_clear.xml: a grey medium with mediumSamplingWeight 1 and strategy single in the laser example's index field"""
    from mitsubaer_amd import host, params as P
    d, spp = host.flatten_xml(SCENE, {"samples": "2", "sigmaS": "0", "sigmaA": "0"})
    assert spp == 2 and d.integrator == P.INTEGRATOR_PTRACER and d.rif_mode == P.RIF_ACOUSTIC
    assert d.strategy == P.STRATEGY_SINGLE and d.medium_sampling_weight == 1.0
    assert list(d.sigma_s) == [0.0] * 3 and list(d.sigma_a) == [0.0] * 3
    d, _ = host.flatten_xml(SCENE, {"samples": "2", "sigmaS": "0.8", "sigmaA": "0.05"})
    assert d.sigma_a[0] == d.sigma_a[1] == d.sigma_a[2] > 0 and d.sigma_s[0] == d.sigma_s[1] == d.sigma_s[2] > 0
