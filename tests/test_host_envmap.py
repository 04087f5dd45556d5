"""The envmap emitter's ABI and Python refusals, without a GPU: mer_emitter keeps its size with the envmap member overlaying radiance,
params.envmap_emitter / capi.validate_emitters refuse what mer_render and mer_envmap_upload refuse."""
import ctypes
import os
import subprocess
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi
from tests import scenes

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
IMG = np.ones((4, 8, 3), np.float32)


def test_emitter_struct_matches_header(tmp_path):
    src = ('#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\nint main(){printf("%zu %zu %zu %zu %zu\\n", sizeof(mer_emitter), '
           'offsetof(mer_emitter, radiance), offsetof(mer_emitter, envmap), offsetof(mer_emitter, env_scale), offsetof(mer_emitter, sampling_weight));return 0;}\n')
    c = tmp_path / "s.c"; c.write_text(src)
    exe = str(tmp_path / "s")
    subprocess.check_call(["cc", "-I", os.path.join(ROOT, "include"), "-o", exe, str(c)])
    size, rad, env, scale, sw = map(int, subprocess.check_output([exe]).split())
    assert size == 92 and env == rad and scale == rad + 4 and sw == rad + 12          # the record keeps its size: the map overlays radiance
    assert ctypes.sizeof(capi.EmitterDesc) == size
    assert capi.EmitterDesc.envmap.offset == env and capi.EmitterDesc.env_scale.offset == scale
    e = capi.EmitterDesc(); e.envmap = 7; e.env_scale = 2.5
    assert (ctypes.c_int32 * (size // 4)).from_buffer(e)[env // 4] == 7
    assert (ctypes.c_float * (size // 4)).from_buffer(e)[scale // 4] == 2.5
    assert P.EMITTER_ENVMAP == 4


def test_envmap_emitter_refusals():
    for img, msg in ((np.zeros((4, 8, 3)), "completely black"), (np.full((4, 8, 3), np.nan), "nan/inf"), (np.full((4, 8, 3), 1e6), "nan/inf"),
                     (np.ones((4, 8)), r"\[height\]\[width\]\[3\]"), (np.ones((0, 8, 3)), r"\[height\]\[width\]\[3\]")):
        with pytest.raises(ValueError, match=msg):
            P.envmap_emitter(img)
    with pytest.raises(ValueError, match="rotation"):
        P.envmap_emitter(IMG, np.diag([1.2, 1.0, 1.0, 1.0]))
    with pytest.raises(ValueError, match="rotation"):
        P.envmap_emitter(IMG, np.diag([-1.0, 1.0, 1.0, 1.0]))                     # a reflection
    with pytest.raises(ValueError, match="scale"):
        P.envmap_emitter(IMG, scale=-1.0)
    with pytest.raises(ValueError, match="samplingWeight"):
        P.envmap_emitter(IMG, sampling_weight=0.0)
    m = np.eye(4); m[:3, 3] = [4, -2, 7]                                           # the translation is ignored
    e = P.envmap_emitter(IMG, m, scale=2.0, sampling_weight=3.0)
    assert e["type"] == P.EMITTER_ENVMAP and e["scale"] == 2.0 and e["sampling_weight"] == 3.0 and e["image"].dtype == np.float32


def test_validate_emitters_refusals():
    e = P.envmap_emitter(IMG)
    capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, env_radiance=[0, 0, 0], emitters=[e, P.point_emitter([0, 0, 0], [1, 1, 1])]))
    with pytest.raises(capi.MerError, match="only contain one environment emitter"):
        capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, emitters=[e]))                 # env_radiance defaults to 1
    with pytest.raises(capi.MerError, match="only contain one environment emitter"):
        capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, env_radiance=[0, 0, 0], emitters=[e, e]))
    bad = dict(e); bad["to_world"] = np.diag([1.0, 2.0, 1.0, 1.0])                 # edited past envmap_emitter's own check
    with pytest.raises(capi.MerError, match="rotation"):
        capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, env_radiance=[0, 0, 0], emitters=[bad]))
    bad = dict(e); bad["sampling_weight"] = -1.0
    with pytest.raises(capi.MerError, match="samplingWeight"):
        capi.validate_emitters(scenes.homogeneous_scene(w=8, h=8, env_radiance=[0, 0, 0], emitters=[bad]))


def test_scene_desc_carries_the_handle():
    """scene_desc fills the entry from the uploaded map's handle and the entry's scale / toWorld rows (no GPU call: a stand-in handle)"""
    class _Vol:
        handle = 42
    m = np.eye(4); m[:3, :3] = [[0, 0, 1], [0, 1, 0], [-1, 0, 0]]
    p = scenes.homogeneous_scene(w=8, h=8, env_radiance=[0, 0, 0], emitters=[P.envmap_emitter(IMG, m, scale=1.5)])
    s = capi.Context.scene_desc(None, p, envmap=_Vol())
    e = s.emitters[0]
    assert s.n_emitters == 1 and e.type == P.EMITTER_ENVMAP and e.envmap == 42 and e.env_scale == 1.5 and e.env_reserved == 0
    assert list(e.to_world) == [0, 0, 1, 0, 0, 1, 0, 0, -1, 0, 0, 0]
