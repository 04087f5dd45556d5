"""K_event hands two pieces of work to where they are cheaper (mer_wavefront.hpp):

 A. the START of a path's free flight (Walk::begin: one RIF gather and the draw of the first segment) runs in K_march -- the record is parked with
    MER_FLAG_INIT, as a spawned side walk's always was -- after Russian roulette and at regeneration;
 B. whether a side-walk slot is busy is read from one byte per slot (8 bytes per path, loaded beside the record) instead of from the state words of six
    different records once the collision is known.

Both leave every sampler stream, every per-path result and every work counter as they were.  Only the plain curved kernels of a steady-state film (the ones
that spawn side walks) do either; per-path output (mer_render_paths), the EXTRA kernels and decomposed films keep every walk's start in K_event, so the
per-path golden below pins nothing new -- it is there so that a later extension of the scheme to those kernels is held to bit equality -- and the FILM of the
default configuration is pinned to the parent commit's as well.

The goldens (tests/golden/kevent_handover_*.npy, kevent_handover_counters.json) were recorded on an MI355X from the library of the parent commit
(4acf910, "Time-resolved fluence: bin light-path deposits by optical path length"), built from its unchanged sources, with the scenes, options, spp and
seeds of this file: render_paths(scene, 0, seed=3) and render_to_host(scene, 0, 8, seed=5) with default options, and the counters of the latter under each
entry of CONFIGS (two runs of each: equal, but for the split of CONFIGS["small_pool"]).  Shapes: 24^3 sigma_t grid and linear RIF, 32 x 32 film, 8 spp, cube boundary, box filter (every
sample adds the same weight to one pixel: the weight channel counts samples).
"""
import json
import os
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi
from tests import scenes

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
SPP, FILM_SEED, PATH_SEED = 8, 5, 3
_BOX = dict(N=24, w=32, h=32, rfilter=P.FILTER_BOX, rfilter_param=0.5)

SCENES = {
    "rk4": lambda: scenes.curved_scene(**_BOX),
    "verlet": lambda: scenes.curved_scene(stepper=P.STEP_VERLET, **_BOX),
    # a medium eight times as dense: a path scatters every step or two while its side walks run some twenty steps to the boundary -- with short passes
    # (CONFIGS["short_passes"]) one walk in six finds the three slots of its kind busy and stays in the path's lane: the busy path of the slot search
    "rk4_dense": lambda: scenes.curved_scene(density_scale=32.0, **_BOX),
    # two-walk estimator: a side walk returns to K_event after each walk, and K_event frees its slot (and clears its busy byte)
    "rk4_woodcock2": lambda: scenes.curved_scene(tr_estimator=P.TR_WOODCOCK2, **_BOX),
    "verlet_woodcock2": lambda: scenes.curved_scene(stepper=P.STEP_VERLET, tr_estimator=P.TR_WOODCOCK2, **_BOX),
    # homogeneous sigma_t on curved rays: begin() takes the sampled-distance branch, and the sampling density it chose is needed at the collision
    "rk4_homogeneous": lambda: scenes.curved_scene(sigma_mode=P.SIGMA_HOMOGENEOUS, **_BOX),
    "verlet_homogeneous": lambda: scenes.curved_scene(sigma_mode=P.SIGMA_HOMOGENEOUS, stepper=P.STEP_VERLET, **_BOX),
    "verlet_homogeneous_maximum": lambda: scenes.curved_scene(sigma_mode=P.SIGMA_HOMOGENEOUS, stepper=P.STEP_VERLET, strategy=P.STRATEGY_MAXIMUM, **_BOX),
    # B-spline RIF whose box is the medium's cube: the spline's limits lie two strides inside it, so EVERY camera ray enters the medium outside them and
    # begin() fails (EV_GATE_FAIL) -- for a PATH, inside K_march
    "bspline_gate": lambda: scenes.bspline_scene(N=24, w=32, h=32, rif=_radial24(), rif_aabb=([-1.0] * 3, [1.0] * 3)),
}
# scheduling: the default (4 pipelines); one pipeline; passes so short that a side walk outlives several scattering events of its path (every path keeps a slot
# of its own, so that the render -- and with it the split between spawned walks and walks in the path's lane -- is the same from run to run); and, on top of
# short passes, a pool of path slots so small that every slot is refilled eight times: a regenerated path finds the busy bytes of its predecessor's walks.
# Which path gets which slot then depends on the order in which waves pop the hit ring, and the split with it -- in the parent too (its two recorded
# runs of "rk4": 6704 + 456 and 6702 + 458) -- so for that configuration the SUM of the two counters is compared, everything else exactly.
CONFIGS = {"default": {}, "pipes1": dict(pipes=1), "short_passes": dict(ksteps=2), "small_pool": dict(nslots=1024, ksteps=4)}
COUNTERS = {"paths": capi.C_PATHS, "eikonal_steps": capi.C_STEPS, "rif_evals": capi.C_RIF_EVALS, "tentative_collisions": capi.C_TENTATIVE, "real_collisions": capi.C_REAL,
            "segments": capi.C_SEGMENTS, "side_walks_spawned": capi.C_SIDE_SPAWNED, "side_walks_in_the_paths_lane": capi.C_SIDE_INLINE}
GOLDEN_SCENES = ("rk4", "verlet")


def _radial24():
    from mitsubaer_amd import synth
    return synth.radial_rif(24)


def _rel_l2(a, b):
    return float(np.linalg.norm(a.astype(np.float64) - b) / max(np.linalg.norm(b.astype(np.float64)), 1e-30))


def render_with_counters(c, sc, opts):
    with c.options(**opts):
        c.counters_reset()
        film = c.render_to_host(sc, 0, SPP, seed=FILM_SEED)
        cnt = c.counters()
    return film, {k: int(cnt[v]) for k, v in COUNTERS.items()}


_ORACLE = {}


@pytest.fixture(scope="module")
def oracle_film(orc):
    """the oracle's film of a scene at the tests' spp and seed: computed once per scene, shared, never written to"""
    def get(name):
        if name not in _ORACLE:
            ref, _ = orc.render(SCENES[name](), 0, SPP, FILM_SEED, nthreads=8)
            ref.setflags(write=False)
            _ORACLE[name] = ref
        return _ORACLE[name]
    return get


@pytest.fixture(scope="module")
def parent_counters():
    with open(os.path.join(GOLDEN, "kevent_handover_counters.json")) as f:
        return json.load(f)


def _film_equals_oracle(ctx, oracle_film, name, config):
    p = SCENES[name]()
    sc, vols = ctx.upload_scene(p)
    film, cnt = render_with_counters(ctx, sc, CONFIGS[config])
    for v in vols:
        v.destroy()
    ref = oracle_film(name)
    assert np.isfinite(film).all()
    assert np.array_equal(film[..., 4], ref[..., 4])       # every sample landed, once: the oracle's weights (box filter: the same table value per sample)
    assert abs(float(film[..., 4].sum()) - 32 * 32 * SPP) < 1e-3 * 32 * 32 * SPP
    err = _rel_l2(film[..., :3], ref[..., :3])
    print("%s / %s: film vs oracle relative L2 %.3e, counters %s" % (name, config, err, cnt))
    assert err < 2e-2                                      # the bar of test_spawned_side_walks_change_no_film (equal spp: a few paths flip a decision on a libm ulp)
    return film, cnt


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["rk4", "verlet", "rk4_dense"])
def test_film_equals_the_oracles(ctx, oracle_film, name, config):
    film, cnt = _film_equals_oracle(ctx, oracle_film, name, config)
    assert cnt["side_walks_spawned"] > 0
    if name == "rk4_dense" and config in ("short_passes", "small_pool"):
        # the busy path of the slot search.  (A walk in the path's lane holds the path up until it ends, and the slots drain meanwhile: the share of such
        # walks saturates far below one -- the parent's is 3711 of 22332 with short passes, 4049 with the small pool on top.)
        assert cnt["side_walks_in_the_paths_lane"] * 10 > cnt["side_walks_spawned"] + cnt["side_walks_in_the_paths_lane"]


@pytest.mark.parametrize("name", GOLDEN_SCENES)
def test_per_path_output_equals_the_parents_bit_for_bit(ctx, name):
    """mer_render_paths against the array the parent commit's library wrote for the same scene, sample index and seed (module docstring).  The per-path
    kernels take neither change, so this pins nothing new (see above)."""
    sc, vols = ctx.upload_scene(SCENES[name]())
    a = ctx.render_paths(sc, 0, seed=PATH_SEED)
    for v in vols:
        v.destroy()
    assert np.array_equal(a, np.load(os.path.join(GOLDEN, "kevent_handover_paths_%s.npy" % name)))


@pytest.mark.parametrize("name", GOLDEN_SCENES)
def test_film_equals_the_parents_up_to_summation_order(ctx, name):
    """the film of the default configuration against the parent commit's (module docstring): the same per-path values reach the same pixels through float
    atomics in another order -- the suite's summation-order bar, rtol 1e-5 / atol 1e-6 -- and the sample counts are exact"""
    sc, vols = ctx.upload_scene(SCENES[name]())
    film, _ = render_with_counters(ctx, sc, CONFIGS["default"])
    for v in vols:
        v.destroy()
    gold = np.load(os.path.join(GOLDEN, "kevent_handover_film_%s.npy" % name))
    print("%s: largest |film - parent's| %.3e" % (name, float(np.abs(film - gold).max())))
    assert np.array_equal(film[..., 3:], gold[..., 3:])
    assert np.allclose(film[..., :3], gold[..., :3], rtol=1e-5, atol=1e-6)


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["rk4_woodcock2", "verlet_woodcock2"])
def test_two_walk_estimator_film_equals_the_oracles(ctx, oracle_film, name, config):
    film, cnt = _film_equals_oracle(ctx, oracle_film, name, config)
    assert cnt["side_walks_spawned"] > 0


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["rk4_homogeneous", "verlet_homogeneous", "verlet_homogeneous_maximum"])
def test_homogeneous_sigma_film_equals_the_oracles(ctx, oracle_film, name, config):
    film, cnt = _film_equals_oracle(ctx, oracle_film, name, config)
    assert cnt["side_walks_spawned"] > 0


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_path_that_fails_the_spline_gate_in_k_march_ends_as_before(ctx, oracle_film, config, parent_counters):
    """every path of this scene fails begin()'s volume-limits gate: transmittance 0, the path is done, its sample still counts -- the oracle's film"""
    film, cnt = _film_equals_oracle(ctx, oracle_film, "bspline_gate", config)
    assert cnt["paths"] == 32 * 32 * SPP and cnt["eikonal_steps"] == 0 and cnt["real_collisions"] == 0
    assert cnt["rif_evals"] == 0 and cnt["segments"] > 0      # free flights were started, and none got as far as its first RIF fetch
    assert cnt == parent_counters["bspline_gate"][config]


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["rk4", "verlet", "rk4_dense", "rk4_woodcock2", "rk4_homogeneous"])
def test_counters_equal_the_parents(ctx, parent_counters, name, config):
    """paths, eikonal steps, RIF evaluations, tentative and real collisions, segments and spawned side walks against the parent commit's counters of the
    same render (module docstring); the split between spawned walks and walks in the path's lane as well, also where most slots are busy
    ("rk4_dense" with short passes).  Where the parent's own split varies from run to run the sum of the two is compared: a refilled slot pool
    (see CONFIGS), and the two-walk estimator with short passes, under which K_event frees a slot while other lanes of the same launch search for one."""
    sc, vols = ctx.upload_scene(SCENES[name]())
    _, cnt = render_with_counters(ctx, sc, CONFIGS[config])
    for v in vols:
        v.destroy()
    gold = parent_counters[name][config]
    print("%s / %s: %s" % (name, config, cnt))
    split = ("side_walks_spawned", "side_walks_in_the_paths_lane")
    for k in COUNTERS:
        if k in split and (config == "small_pool" or ("woodcock2" in name and config != "default" and config != "pipes1")):
            assert cnt[split[0]] + cnt[split[1]] == gold[split[0]] + gold[split[1]]
            continue
        assert cnt[k] == gold[k], k


KINDS = {1: "slot", 2: "queue segment overflow", 3: "queue item", 4: "hit ring", 5: "film", 6: "path_out", 14: "side-walk busy bytes"}


@pytest.fixture(scope="module")
def cctx():
    c = capi.Context(0, check=True)
    en, *_ = c.debug_bounds()
    assert en, "libmer_check.so was built without -DMER_BOUNDS_CHECK"
    yield c
    c.close()


@pytest.mark.parametrize("config", sorted(CONFIGS))
@pytest.mark.parametrize("name", ["rk4", "verlet", "rk4_woodcock2"])
def test_bounds_checking_build_reports_nothing(cctx, ctx, name, config):
    """the same renders through libmer_check.so: no index out of range -- the busy bytes (check kind 14) included -- and the product build's film"""
    sc, vols = cctx.upload_scene(SCENES[name]())
    film, cnt = render_with_counters(cctx, sc, CONFIGS[config])
    en, n, kind, idx, lim = cctx.debug_bounds()
    for v in vols:
        v.destroy()
    assert n == 0, "%d out-of-range accesses; first: %s index %d, limit %d" % (n, KINDS.get(kind, kind), idx, lim)
    s2, v2 = ctx.upload_scene(SCENES[name]())
    ref, cref = render_with_counters(ctx, s2, CONFIGS[config])
    for v in v2:
        v.destroy()
    assert np.array_equal(film[..., 3:], ref[..., 3:]) and np.allclose(film[..., :3], ref[..., :3], rtol=2e-4, atol=2e-5)
    assert cnt["paths"] == cref["paths"] and cnt["real_collisions"] == cref["real_collisions"]
