"""The four light-path kernels -- K_ptracer, K_fluence (steady and time-resolved), K_fluence_track, K_exitance -- share one walk (mer_lightpath.hpp).
This file holds every family, on a scene per kind of instantiation, to what the kernels computed BEFORE they shared it.

The goldens (tests/golden/lightpath_parent_<scene>.npy, lightpath_parent_counters.json) were recorded on an MI355X from the library of the parent
commit (0b45040, "Exitance maps: where and when light paths leave the medium"), built from its unchanged sources and selected through MER_LIB, with
the scenes, shapes and seed of this file (record() below is what the recorder called).  They were recorded twice.  The two recordings agree exactly
in every integer -- the eight work counters, totals[0] (paths), totals[7] (ended), the exitance map's totals[14] (deposits) -- and those are
compared exactly; nothing had to be demoted.  Sums and the remaining totals are float64 atomics of one set of deposits in another order: rtol 1e-9,
the suite's RTOL_SUM (test_gpu_exitance.py has the derivation).  The film is float32 atomics in another order: the rtol 1e-4 / atol 1e-5 of
test_shards_add_up_to_the_whole.

Shapes, the smallest that reach every shared step: a 16 x 16 film (one partial 32 x 32 tile: three quarters of the work ids hold no path and idle
through the wave-uniform loops), 4 samples per pixel (1024 paths), an 8^3 fluence box, a 4 x 4 exitance map, and 4 frames for each timed family
over a window that starts with the entry into the shape and ends before the last deposits.  Every scene but `point_inside` is lit by a collimated
beam from outside the shape -- entry, one depth, and with rr_depth = 1 the roulette at entry.
"""
import json
import os
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, synth
from tests import test_exitance64 as T
from tests import test_gpu_exitance as TE

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPP, SEED = 4, 11
PATHS = TE.W * TE.H * SPP
BOX = ((8, 8, 8), (-1, -1, -1), (1, 1, 1))
FRAMES = 4
FLUENCE_WINDOW = dict(t_min=2.0, t_bin=0.5)              # the beam enters after 2 units; a path of several flights runs past 4
EXITANCE = dict(frames=FRAMES, t_min=2.0, t_bin=1.0, cos_min=0.3)
RTOL_SUM = TE.RTOL_SUM
COUNTERS = (capi.C_PATHS, capi.C_STEPS, capi.C_RIF_EVALS, capi.C_TENTATIVE, capi.C_REAL, capi.C_SEGMENTS, capi.C_NEE, capi.C_ACTIVE_LANES)
FAMILIES = ("ptracer", "fluence", "fluence_time", "fluence_track", "exitance")
EXACT_TOTALS = {"fluence": (0, 7), "fluence_time": (0, 7), "fluence_track": (0, 7), "exitance": (0, 7, 14)}

_H = 0.05
_AC = dict(rif_mode=P.RIF_ACOUSTIC, ac_n_o=1.33, ac_n_max=0.08, ac_k_r=4.0)
SCENES = {
    "straight_homogeneous": lambda: TE._base(rr_depth=1),
    "straight_grid": lambda: TE._grid(rr_depth=1),
    "trilinear_verlet": lambda: TE._grid(rr_depth=1, rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=_H, stepper=P.STEP_VERLET),
    "trilinear_rk4": lambda: TE._base(rr_depth=1, rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=_H, stepper=P.STEP_RK4),
    # the spline's limits lie two strides inside its box: +-1.6 keeps the cube within them
    "bspline": lambda: TE._grid(rr_depth=1, rif_mode=P.RIF_BSPLINE3, rif=synth.radial_rif(16, (-1.6,) * 3, (1.6,) * 3), rif_aabb=([-1.6] * 3, [1.6] * 3),
                                stepsize=_H, stepper=P.STEP_VERLET),
    "acoustic": lambda: TE._base(rr_depth=1, stepsize=_H, stepper=P.STEP_RK4, **_AC),
    "point_inside": lambda: TE._base(rr_depth=1, emitters=[P.point_emitter([0.1, -0.2, 0.3], [TE.INTENSITY] * 3)]),
    "beam_misses": lambda: TE._base(rr_depth=1, emitters=[TE._beam(o=[3.0, 3.0, -3.0])]),
    "max_depth_2": lambda: TE._base(rr_depth=1, max_depth=2),
}


def record(c, name):
    """one render of every family on the scene: {family: (counters [8], arrays ...)} -- film for the light tracer, (sums, totals) for the others"""
    sc, vols = c.upload_scene(SCENES[name](), layout=capi.LAYOUT_DENSE)
    handles = {"fluence": c.fluence_create(*BOX), "fluence_time": c.fluence_time_create(*BOX, frames=FRAMES, **FLUENCE_WINDOW),
               "fluence_track": c.fluence_track_create(*BOX)}
    he = c.exitance_create(sc.boundary, T.RES, **EXITANCE)
    out = {}

    def counted(render):
        c.counters_reset()
        got = render()
        cnt = c.counters()
        return [int(cnt[k]) for k in COUNTERS], got
    try:
        cnt, film = counted(lambda: c.render_to_host(sc, 0, SPP, seed=SEED))
        out["ptracer"] = (cnt, film)
        for fam, h in handles.items():
            cnt, _ = counted(lambda: c.render_fluence(sc, h, 0, SPP, seed=SEED))
            out[fam] = (cnt,) + tuple(c.fluence_time_read(h) if fam == "fluence_time" else c.fluence_read(h))
        cnt, _ = counted(lambda: c.render_exitance(sc, he, 0, SPP, seed=SEED))
        out["exitance"] = (cnt,) + tuple(c.exitance_read(he))
    finally:
        for h in handles.values():
            c.fluence_destroy(h)
        c.exitance_destroy(he)
        for v in vols:
            v.destroy()
    return out


def pack(out):
    """the arrays of record() as one float64 vector (the film's float32 values are exact in it), in the order of FAMILIES"""
    return np.concatenate([np.asarray(a, np.float64).ravel() for fam in FAMILIES for a in out[fam][1:]])


@pytest.fixture(scope="module")
def parent_counters():
    with open(os.path.join(GOLDEN, "lightpath_parent_counters.json")) as f:
        return json.load(f)


_RUNS = {}


@pytest.fixture(scope="module")
def run(ctx):
    """the renders of a scene, once per scene, with the parent's arrays cut to the same shapes: {family: (counters, arrays, parent's arrays)}"""
    def get(name):
        if name not in _RUNS:
            out = record(ctx, name)
            gold = np.load(os.path.join(GOLDEN, "lightpath_parent_%s.npy" % name))
            assert gold.shape == pack(out).shape
            at, res = 0, {}
            for fam in FAMILIES:
                cut = []
                for a in out[fam][1:]:
                    cut.append(gold[at:at + a.size].reshape(a.shape)); at += a.size
                res[fam] = (out[fam][0], out[fam][1:], cut)
            _RUNS[name] = res
        return _RUNS[name]
    return get


@pytest.mark.parametrize("family", FAMILIES)
@pytest.mark.parametrize("name", sorted(SCENES))
def test_equals_the_parent_commit(run, parent_counters, name, family):
    cnt, got, gold = run(name)[family]
    print(name, family, "counters", cnt, "parent's", parent_counters[name][family])
    assert cnt == parent_counters[name][family]
    assert cnt[0] == PATHS
    if family == "ptracer":
        film, gfilm = got[0], gold[0]
        print("largest |film - parent's| %.3e" % float(np.abs(film - gfilm).max()))
        assert np.isfinite(film).all()
        assert np.array_equal(film[..., 3:], gfilm[..., 3:])           # alpha and weight: one unit per path
        np.testing.assert_allclose(film[..., :3], gfilm[..., :3], rtol=1e-4, atol=1e-5)
        return
    (sums, tot), (gsums, gtot) = got, gold
    print("totals", list(tot), "parent's", list(gtot))
    assert np.isfinite(sums).all() and np.isfinite(tot).all()
    for k in EXACT_TOTALS[family]:
        assert tot[k] == gtot[k], k
    np.testing.assert_allclose(tot, gtot, rtol=RTOL_SUM, atol=0)
    np.testing.assert_allclose(sums, gsums, rtol=RTOL_SUM, atol=0)


def test_the_scenes_reach_what_they_are_there_for(run):
    """guards the goldens' coverage: entry with the roulette at work, the miss, the window's cut, and deposits at all"""
    t = {name: {fam: run(name)[fam][1][1] for fam in FAMILIES[1:]} for name in ("straight_homogeneous", "beam_misses", "point_inside", "max_depth_2")}
    s = t["straight_homogeneous"]
    assert 0 < s["exitance"][14] < PATHS                                          # rr_depth 1: the roulette ends paths, others leave inside the cone and the window
    assert s["fluence_time"][8] > 0 and s["exitance"][8] > 0 and s["exitance"][11] > 0     # out of the window; outside the cone
    m = t["beam_misses"]
    assert m["exitance"][14] == 0 and m["exitance"][4] == m["exitance"][1] == PATHS * T.POWER and m["fluence"][1] == PATHS * T.POWER
    assert t["point_inside"]["exitance"][4] == 0 and t["point_inside"]["exitance"][14] > 0
    assert run("straight_homogeneous")["fluence"][0][4] > run("max_depth_2")["fluence"][0][4] > 0      # real collisions: max_depth 2 cuts the paths short
