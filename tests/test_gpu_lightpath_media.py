"""The light-path kernels (K_fluence, its time-resolved and track-length kinds, K_exitance, K_ptracer) in media where the three channels differ
and where delta tracking meets null collisions -- what the grey, constant-density scenes of tests/test_gpu_fluence*.py,
test_gpu_exitance.py and test_gpu_ptracer.py cannot see: the distance-sampling strategies with a channel-dependent sigma_t, the per-channel
weights transmittance / pdfSuccess and transmittance / pdfFailure, the three channels through wave_deposit, and Walk::on_arrived returning
"null collision".

The oracle (tests/test_lightpath64.py): channel c of a chromatic homogeneous render equals, in expectation, the GREY float64 references run
with channel c's sigma_s, sigma_a and power; and tests/lightpath64.py, the float64 restatement with an RGB throughput, which is itself held
to those references and, for the sigma_t ramp, to closed forms.  Scenes, shapes and checks are that module's.

Set-up: the helpers of the four families' GPU tests -- 16 x 16 x 64 = 16 384 paths per batch, K = 16 batches with seeds s0 + j, the dense
layout, the beam from (0.2, 0.1, -3) along +z with the power (5, 3, 8), medium_sampling_weight = 1 unless said.  Statistics: the project's
bar -- at most 1 + 1 % of the cells beyond 4 sigma, totals within 4 sigma.  No path ends by "no forward progress" with these seeds
(totals[7] == 0, as test_curved_scattering_balances explains).

Measured on the MI355X, channel 0, before and after the escaped weight took the factor transmittance / pdfFailure (LightPath::weigh_exit):
escaped against grey z = 397.7 / 280.3 / 152.9 (balance / maximum / single) before, 0.81 / 0.36 / 0.26 after; the steady map 96 / 95 / 93 of 96
cells beyond 4 sigma before, 0 - 1 after; medium_sampling_weight = 0.7, balance z = 388.3 before, 0.46 after; the curved map 96 of 96 cells
before, 0 after, and the curved escaped total z = 13.0 with the factor taken at W.dist, 0.24 / 0.50 / 0.32 per channel with half the leaving
step added.  The ramp, the film and the cells of the collision, time and track grids passed before as well: they do not depend on it."""
import functools
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi
from tests import scenes
from tests import fluence64 as F
from tests import exitance64 as E
from tests import ptracer64 as pt
from tests import test_lightpath64 as L
from tests import test_ptracer64 as T64
from tests import test_gpu_fluence as TG
from tests import test_gpu_fluence_time as TGT
from tests import test_gpu_fluence_track as TGK
from tests import test_gpu_exitance as TGE
from tests import test_gpu_ptracer as TP
from tests.test_fluence_time64 import SC

pytestmark = pytest.mark.gpu
K, PATHS, RTOL_SUM = TG.K, TG.PATHS, TG.RTOL_SUM
assert (K, PATHS) == (L.K, L.PATHS)
STRATEGY = {"balance": P.STRATEGY_BALANCE, "maximum": P.STRATEGY_MAXIMUM, "single": P.STRATEGY_SINGLE}
BEAM = P.collimated_emitter(TP._beam_frame(TG.BEAM_O, TG.BEAM_D), list(L.POWER3))


def _homogeneous(strategy, chroma, **kw):
    c = L.CHROMA[chroma]
    return TG._base(sigma_s=list(c["sigma_s"]), sigma_a=list(c["sigma_a"]), g=L.G, strategy=STRATEGY[strategy], emitters=[BEAM], **kw)


def _ramp(albedo=L.RAMP["albedo"], **kw):
    """sigma_t from 0.5 at z = -1 to 4 at z = +1: a 2 x 2 x 2 density grid, 0.125 on the z = -1 nodes and 1 on the z = +1 nodes, scale 4"""
    dens = np.full((2, 2, 2), L.RAMP["s_lo"] / L.RAMP["s_hi"], np.float32); dens[1] = 1.0
    base = dict(sigma_mode=P.SIGMA_GRID, density=dens, density_scale=L.RAMP["s_hi"], albedo=list(albedo), g=L.G, emitters=[BEAM])
    base.update(kw)
    return TG._base(**base)


def _render(ctx, p, seed0, kinds, tmap=None):
    """the kinds asked for (grid / tgrid / track / emap; tmap = the map's window and cone) in the form of lightpath64.render's result"""
    out = {}
    for i, kind in enumerate(kinds):
        s0 = seed0 + 20 * i
        if kind == "grid":
            out["grid"], out["grid_totals"] = TG._batches(ctx, p, s0, res=L.GRID["res"])
        elif kind == "tgrid":
            out["tgrid"], out["tgrid_totals"] = TGT._batches(ctx, p, s0, **SC)
        elif kind == "track":
            out["track"], out["track_totals"] = TGK._batches(ctx, p, s0, res=L.GRID["res"])
        else:
            desc = {k: v for k, v in (tmap or {}).items() if k != "res"}
            out["emap"], out["emap_totals"] = TGE._batches(ctx, p, s0, res=L.MAP["res"], **desc)
        t = out[("emap" if kind in ("emap", "tmap") else kind) + "_totals"]
        assert np.all(t[:, 0] == PATHS) and np.all(t[:, 7] == 0), kind
    return out


def _map_identity(out):
    """sum(sums) + missed + rejected + late == escaped, per batch and channel"""
    TGE._identity(out["emap"], out["emap_totals"], rtol=RTOL_SUM)


# ---- 1. chromatic homogeneous media ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("strategy", ["balance", "maximum", "single"])
def test_chromatic_homogeneous_grids(ctx, strategy):
    """the collision grid and the time grid (window SC): every channel's cells and its escaped (and
    out-of-window) total against the grey reference of that channel and against lightpath64; the per-channel energy balance; the channels
    differ in the beam's column"""
    chroma, tchroma = L.CASES[strategy], L.TGRID_CASES[strategy]
    kinds = ("grid",)
    out = _render(ctx, _homogeneous(strategy, chroma), 1100, kinds)
    L.check_against_grey(out, chroma, kinds, "GPU " + strategy)
    L.check_against(out, L.chroma_ref(strategy), kinds, "GPU " + strategy)
    tout = _render(ctx, _homogeneous(strategy, tchroma), 1200, ("tgrid",))
    L.check_against_grey(tout, tchroma, ("tgrid",), "GPU " + strategy)
    L.check_against(tout, L.tgrid_ref(strategy), ("tgrid",), "GPU " + strategy)
    sa = L.CHROMA[chroma]["sigma_a"]
    L.check_balance(out["grid"], out["grid_totals"], sa, "GPU %s grid" % strategy)
    L.check_balance(tout["tgrid"], tout["tgrid_totals"], L.CHROMA[tchroma]["sigma_a"], "GPU %s time grid" % strategy, extra=tout["tgrid_totals"][:, 8:11])
    L.check_channels_differ(L.column(out["grid"]), "GPU " + strategy)
    L.check_channels_differ(L.column(tout["tgrid"].sum(1)), "GPU %s time grid" % strategy)


_TRACK = {}


@pytest.mark.parametrize("c", [0, 1, 2])
def test_chromatic_track_grid(ctx, c):
    """the track-length grid under single (mild chroma), rendered once; one channel per case, because a grey float64 track reference takes
    5 s: the channel's cells and escaped total against its grey reference and against lightpath64; with channel 0 also the balance of
    all three"""
    if "out" not in _TRACK:
        _TRACK["out"] = _render(ctx, _homogeneous("single", "mild"), 1150, ("track",))
    out = _TRACK["out"]
    L.check_against_grey(out, "mild", ("track",), "GPU single", channels=(c,))
    ref = L.chroma_ref("single", "track")
    L._cells(out["track"][..., c], ref["track"][..., c], "GPU single track channel %d against lightpath64" % c)
    L._total(out["track_totals"][:, 1 + c], ref["track_totals"][:, 1 + c], "GPU single track channel %d escaped against lightpath64" % c)
    if c == 0:
        L.check_balance(out["track"], out["track_totals"], L.CHROMA["mild"]["sigma_a"], "GPU single track grid")
        L.check_channels_differ(L.column(out["track"]), "GPU single track")


@pytest.mark.parametrize("strategy", ["balance", "maximum", "single"])
def test_chromatic_homogeneous_maps(ctx, strategy):
    """the exitance map of the cube, steady and timed with a cone (TMAP): every channel's keys and the escaped, late and rejected totals
    against the grey reference of that channel and lightpath64; every escaping path in exactly one total"""
    chroma = L.CASES[strategy]
    p = _homogeneous(strategy, chroma)
    out = _render(ctx, p, 2300, ("emap",))                 # not 1300: seed 1310 ends one path under balance by a zero-length flight
    L.check_against_grey(out, chroma, ("emap",), "GPU " + strategy)
    L.check_against(out, L.chroma_ref(strategy), ("emap",), "GPU " + strategy)
    _map_identity(out)
    assert np.all(out["emap_totals"][:, 4:7] == 0) and np.all(out["emap_totals"][:, 8:14] == 0)
    tout = _render(ctx, p, 1400, ("tmap",), tmap=L.TMAP)
    L.check_against_grey(tout, chroma, ("tmap",), "GPU " + strategy)
    L.check_against(tout, L.chroma_ref(strategy, "tmap"), ("tmap",), "GPU " + strategy)
    _map_identity(tout)
    assert np.all(tout["emap_totals"][:, 8:14] > 0)
    m = out["emap"][:, 0, TGE.T.BEAM_FACE].reshape(K, -1, 3)
    L.check_channels_differ(m, "GPU %s map, face +z" % strategy)


# ---- 2. one curved instantiation -------------------------------------------------------------------------------------------------------

CURVED_MAP = dict(res=L.MAP["res"], frames=6, t_min=2.0, t_bin=1.5, cos_min=0.2)       # test_gpu_exitance.py's test_constant_rif_grid_matches_rif_const


@functools.lru_cache(maxsize=None)
def _straight_133(c):
    s = L.CHROMA["strong"]
    return E.render(L.beam(c), s["sigma_s"][c], s["sigma_a"][c], L.G, E.CUBE, n=1.33, paths=PATHS, batches=K, seed=130 + c, rr_depth=5, **CURVED_MAP)


def test_curved_chromatic_map_matches_the_straight_grey_references(ctx):
    """a constant 1.33 index grid through the curved kernels (RK4, stepsize 0.05), the strong chroma under balance: the flight that leaves
    is weighed at W.dist.  Per channel the escaped total and the map, per cell over the window (not per frame: test_gpu_exitance.py's
    test_constant_rif_grid_matches_rif_const has the reason), against the straight grey float64 reference with n = 1.33"""
    rif = np.full((16, 16, 16), 1.33, np.float32)
    p = _homogeneous("balance", "strong", rif_mode=P.RIF_TRILINEAR, rif=rif, stepsize=0.05, stepper=P.STEP_RK4)
    out = _render(ctx, p, 1500, ("tmap",), tmap=CURVED_MAP)
    _map_identity(out)
    for c in range(3):
        r, rt = _straight_133(c)
        a, b = out["emap"][..., c].sum(1), r.sum(1)
        E.bar(a.mean(0), a.std(0, ddof=1) / np.sqrt(K), b.mean(0), b.var(0, ddof=1) / K, what="GPU curved map channel %d" % c)
        E.total_bar(out["emap_totals"][:, 1 + c], rt[:, 1].mean(), rt[:, 1].var(ddof=1) / K, what="GPU curved escaped channel %d" % c)
        E.total_bar(out["emap_totals"][:, 11 + c], rt[:, 11].mean(), rt[:, 11].var(ddof=1) / K, what="GPU curved rejected channel %d" % c)


# ---- 3. the sigma_t ramp: null collisions ----------------------------------------------------------------------------------------------

def test_ramp_matches_lightpath64(ctx):
    """sigma_t 0.5 ... 4 under a majorant of 4, albedo (0.9, 0.6, 0.3): the collision grid, the time grid, the track grid and the map per
    channel against lightpath64, whose free flights invert the optical depth in closed form; roughly half of the tentative collisions are
    null (the work counters)"""
    p = _ramp()
    ctx.counters_reset()
    out = _render(ctx, p, 1600, ("grid", "tgrid", "track", "emap"))
    cnt = ctx.counters()
    print("ramp: tentative %d, real %d" % (cnt[capi.C_TENTATIVE], cnt[capi.C_REAL]))
    assert cnt[capi.C_TENTATIVE] > 1.5 * cnt[capi.C_REAL] > 0
    L.check_against(out, L.ramp_ref(L.RAMP_SEEDS[0]), ("grid", "tgrid", "track", "emap"), "GPU ramp")
    _map_identity(out)
    assert (out["grid"].mean(0) > 0).all()
    L.check_channels_differ(L.column(out["grid"]), "GPU ramp")
    L.check_channels_differ(L.column(out["track"]), "GPU ramp track")


def test_absorbing_ramp_is_the_closed_form(ctx):
    out = _render(ctx, _ramp(albedo=(0.0,) * 3), 1700, ("grid", "track"))
    L.check_absorbing_ramp(out, "GPU")


def test_ramp_with_an_albedo_grid_balances(ctx):
    """ALBEDO_GRID, the RGB grid of tests/scenes.py: no per-cell reference of its own is needed for the balance -- the power that escapes
    per channel is the emitted power less what lightpath64 absorbs at its collisions with the interpolated albedo; the cells are held to
    lightpath64 as well"""
    p = _ramp(albedo_mode=P.ALBEDO_GRID, albedo_grid=scenes.rgb_albedo(8))
    out = _render(ctx, p, 1750, ("grid",))
    ref = L.ramp_albedo_grid_ref()
    for c in range(3):
        absorbed = ref["absorbed"][:, c]
        F.total_bar(out["grid_totals"][:, 1 + c], PATHS * L.POWER3[c] - absorbed.mean(), absorbed.var(ddof=1) / K, what="GPU albedo grid escaped channel %d" % c)
    L.check_against(out, ref, ("grid",), "GPU albedo grid")


# ---- 4. medium_sampling_weight below 1 -------------------------------------------------------------------------------------------------

def test_medium_sampling_weight_below_one_balances(ctx):
    """grey, medium_sampling_weight = 0.7: escaped + absorbed = emitted per channel, and the grid and the map against lightpath64"""
    p = TG._base(medium_sampling_weight=0.7, emitters=[BEAM])
    out = _render(ctx, p, 1800, ("grid", "emap"))
    L.check_balance(out["grid"], out["grid_totals"], (TG.T.SIGMA_A,) * 3, "GPU weight 0.7")
    L.check_against(out, L.msw_ref(), ("grid", "emap"), "GPU weight 0.7")
    _map_identity(out)


# ---- 5. the film's colour --------------------------------------------------------------------------------------------------------------

FILM_I = (1.0, 0.8, 0.5)


@functools.lru_cache(maxsize=None)
def _film_ref(c):
    s = L.CHROMA["strong"]
    return pt.render(pt.point(TP.PIN, FILM_I[c]), s["sigma_s"][c], s["sigma_a"][c], T64.G, TP.W, TP.H, TP.FOV, TP.CAM, spp=1024, batches=32, seed=70 + c,
                     full=True)[..., 0]


def test_film_channels_match_their_grey_light_tracer(ctx):
    """K_ptracer on the strong chroma under balance, a point emitter of intensity (1, 0.8, 0.5) inside the cube: each film channel against
    the float64 light tracer run grey with that channel's numbers (64 renders of 64 samples, as test_light_tracing_equals_path_tracing)"""
    s = L.CHROMA["strong"]
    KE = 64
    p = TP._base(emitters=[P.point_emitter(TP.PIN, list(FILM_I))], sigma_s=list(s["sigma_s"]), sigma_a=list(s["sigma_a"]), strategy=P.STRATEGY_BALANCE)
    lt, film = TP._renders(ctx, p, 64, 1900, k=KE)
    assert np.all(film[..., -1] == 64)
    for c in range(3):
        a = lt[:, :, :, 0, c]
        r = _film_ref(c)                                                   # (32, H, W): the films of the reference's batches
        TP._bar(a.mean(0), a.std(0, ddof=1) / np.sqrt(KE), r.mean(0), r.var(0, ddof=1) / len(r), what="film channel %d" % c)
        TP._total_bar(a.sum((1, 2)), r.sum((1, 2)).mean(), r.sum((1, 2)).var(ddof=1) / len(r), what="film total channel %d" % c)
    tot = lt[:, :, :, 0, :].sum((1, 2))
    for a, b in ((0, 1), (0, 2), (1, 2)):
        assert abs(tot[:, a].mean() - tot[:, b].mean()) > 10 * np.sqrt((tot[:, a].var(ddof=1) + tot[:, b].var(ddof=1)) / KE)
