"""Frequency-domain exitance maps (mer_exitance_fd_create, the FD kind of K_exitance) on the GPU: the deterministic phase of an unscattered
beam's exit, same-seed identities against the steady and the time-gated map on one scene per kind of instantiation, the float64 restatement
tests/fd64.py in a scattering and in a chromatic medium, and the interface: shards, clear / accumulate, the bounds-checking build, the
refusals, `mer_render --exitance --frequencies`.

The set-up, the bar and the helpers are those of tests/test_gpu_fluence_fd.py.

Measured on an MI355X (this file's seeds): the exit phase |(cos, sin) - exact| 6.4e-8 / 1.5e-8 (n = 1, k = 0.7 / 3.0) and 1.9e-7 / 5.5e-7
(n = 1.4) against bounds 9.8e-7 / 2.6e-6 and 1.1e-6 / 3.1e-6; the identities: modulus / steady at most 1.000000000, DFT difference at most
1.000 of the bound (max_depth_2: the unscattered beam leaves at l = 4.0, on a bin edge; |e^{ia} - e^{ib}| < |a - b| keeps it inside);
against float64: 0 of 480 (3.01), chromatic 0 of 1440 (3.31)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host
from tests import test_exitance64 as T
from tests import test_fd64 as TF
from tests import test_gpu_exitance as TE
from tests import test_gpu_fluence_fd as TG
from tests import test_gpu_lightpath_parent as TL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, PATHS, SPP, RTOL_SUM, KS, T_BIN = TG.K, TG.PATHS, TG.SPP, TG.RTOL_SUM, TG.KS, TG.T_BIN
COS_MIN = 0.3                                  # the cone of the identity tests, tests/test_gpu_lightpath_parent.py's


def _batches(ctx, p, seed0, res=T.RES, ks=KS, k=K, cos_min=0.0):
    """k batches with seeds seed0 + j into one map, cleared in between: raw sums (k, n_freq, 2, faces, res_v, res_u, 3), totals (k, 16)"""
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.exitance_fd_create(sc.boundary, res, ks, cos_min)
    sums, totals = [], []
    try:
        for j in range(k):
            ctx.exitance_clear(h)
            ctx.render_exitance(sc, h, 0, SPP, seed=seed0 + j)
            s, t = ctx.exitance_fd_read(h)
            assert np.isfinite(s).all() and np.isfinite(t).all() and t[15] == 0 and np.all(t[8:11] == 0)
            sums.append(s); totals.append(t)
    finally:
        ctx.exitance_destroy(h)
        for v in vols:
            v.destroy()
    return np.array(sums), np.array(totals)


# ---- 4. the deterministic exit phase -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1.0, 1.4])
def test_unscattered_beam_exits_with_the_phase_of_its_path(ctx, n):
    """pure absorber: the beam's cell holds N P (cos phi, sin phi), N = totals[14], phi = k (2 + 2 n), within 2^-21 (the phase arithmetic's
    contract) + k (2 + 2 n) 3 x 2^-24 (two float32 roundings of l, one of the product); every other cell of every plane is exactly 0.0; the
    real plane of k = 0 obeys sum + missed + rejected = escaped"""
    sums, tot = _batches(ctx, TG.absorber(n), 3100, k=4)
    g = TG.grey(sums)
    assert g.shape == (4, 3, 2, 6, 4, 4)
    on = np.zeros(g.shape[1:], bool); on[:, :, T.BEAM_FACE, T.BEAM_IV, T.BEAM_IU] = True
    assert np.all(g[:, ~on] == 0.0), "exits off the beam's cell"
    assert np.all(g[:, 0, 1] == 0.0), "the imaginary plane of k = 0"
    # (totals[7] is the walk's own: a flight of length 0 ends a path without progress, once in these 65 536)
    assert np.all(tot[:, 14] > 0) and np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:7] == 0) and np.all(tot[:, 8:14] == 0)
    for j, k in enumerate(KS):
        phi = k * (2.0 + 2.0 * n)
        unit = g[:, j, :, T.BEAM_FACE, T.BEAM_IV, T.BEAM_IU] / (tot[:, 14] * T.POWER)[:, None]
        err = float(np.abs(unit - np.array([np.cos(phi), np.sin(phi)])).max())
        bound = 2.0 ** -21 + phi * 3 * 2.0 ** -24
        print("n %.1f, k %.1f: |(cos, sin) - exact| %.3e, bound %.3e" % (n, k, err, bound))
        assert err <= bound
    np.testing.assert_array_equal(g[:, 0, 0].reshape(4, -1).sum(1) + tot[:, 4] + tot[:, 11], tot[:, 1])      # sums of P: exact in float64


# ---- 5. same-seed identities -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(TL.SCENES))
def test_same_seed_identities(ctx, name):
    """one scene per kind of instantiation, 1024 paths, a 4 x 4 map with a cone: the frequency-domain handle against the steady and the
    time-gated handle of the same scene, shard and seed"""
    p, l_max = TG.bounded(name)
    frames = int(np.ceil(l_max / T_BIN))
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    hs = ctx.exitance_create(sc.boundary, T.RES, cos_min=COS_MIN)
    ht = ctx.exitance_create(sc.boundary, T.RES, frames=frames, t_min=0.0, t_bin=T_BIN, cos_min=COS_MIN)
    hf = ctx.exitance_fd_create(sc.boundary, T.RES, KS, COS_MIN)
    try:
        cs = TG.counted(ctx, lambda: ctx.render_exitance(sc, hs, 0, TL.SPP, seed=TL.SEED))
        ct = TG.counted(ctx, lambda: ctx.render_exitance(sc, ht, 0, TL.SPP, seed=TL.SEED))
        cf = TG.counted(ctx, lambda: ctx.render_exitance(sc, hf, 0, TL.SPP, seed=TL.SEED))
        (steady, ts), (timed, tt), (fd, tf) = ctx.exitance_read(hs), ctx.exitance_read(ht), ctx.exitance_fd_read(hf)
    finally:
        for h in (hs, ht, hf):
            ctx.exitance_destroy(h)
        for v in vols:
            v.destroy()
    print(name, "counters", cf, "totals", list(tf))
    assert cf == cs == ct and cf[0] == TL.PATHS
    assert tf[0] == ts[0] == TL.PATHS and tf[7] == ts[7] and tf[14] == ts[14]
    np.testing.assert_allclose(tf, ts, rtol=RTOL_SUM, atol=0)
    assert np.all(tt[8:11] == 0), "exits outside the timed window: the bound on the path length does not hold"
    if name != "beam_misses":
        assert steady.sum() > 0 and np.abs(fd[1:, 1]).sum() > 0
    if name == "straight_homogeneous":
        assert tf[11] > 0                                                  # the cone was at work
    worst, mod = TG.check_identities(fd, steady[0], timed, KS, frames * T_BIN, name)
    print("%s: largest DFT difference / bound %.3f, largest modulus / steady %.9f" % (name, worst, mod))


# ---- 7. against the float64 restatement --------------------------------------------------------------------------------------------------

def test_scattering_medium_matches_float64(ctx):
    """sigma_s 2, sigma_a 0.1, g 0.8, n 1.4 on a 4 x 4 map: every value of both planes under the bar"""
    r = TF.scattering_ref()
    sums, tot = _batches(ctx, TG.scattering(), 3300)
    g = TG.grey(sums)[..., None]
    assert g.shape == r["map"].shape
    n, zmax = TF.compare(g, tot, r["map"], r["map_totals"], "GPU map", (1, 14))
    print("scattering map: %d values compared, max z %.2f" % (n, zmax))
    assert n == 576 - 96 and np.all(g[:, 0, 1] == 0.0)
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:7] == 0) and np.all(tot[:, 8:14] == 0)


def test_chromatic_medium_matches_float64(ctx):
    """three different sigma_t under strategy single: the exit weight goes through weigh_exit, tau_c / pdfFailure per channel"""
    r = TF.chromatic_ref()
    sums, tot = _batches(ctx, TG.chromatic(), 3400)
    assert sums.shape == r["map"].shape
    n, zmax = TF.compare(sums, tot, r["map"], r["map_totals"], "GPU chromatic map", (1, 2, 3, 14))
    print("chromatic map: %d values compared, max z %.2f" % (n, zmax))
    assert n == 3 * (576 - 96)
    face = sums[:, 0, 0, T.BEAM_FACE].sum((0, 1, 2))
    assert not np.isclose(face[0], face[1], rtol=1e-3) and not np.isclose(face[1], face[2], rtol=1e-3)


# ---- 8. the interface --------------------------------------------------------------------------------------------------------------------

def test_half_shards_add_up_and_the_map_accumulates(ctx):
    sc, _ = ctx.upload_scene(TG.scattering())
    h = ctx.exitance_fd_create(sc.boundary, T.RES, KS, COS_MIN)
    try:
        ctx.render_exitance(sc, h, 0, SPP, seed=9)
        whole, tw = ctx.exitance_fd_read(h)
        parts = []
        for begin in (0, 32):
            ctx.exitance_clear(h)
            z, tz = ctx.exitance_fd_read(h)
            assert not z.any() and not tz.any()
            ctx.render_exitance(sc, h, begin, 32, seed=9)
            parts.append(ctx.exitance_fd_read(h))
        assert parts[0][1][0] == parts[1][1][0] == PATHS // 2 and tw[0] == PATHS
        assert np.abs(parts[0][0]).sum() > 0 and not np.array_equal(parts[0][0], parts[1][0])
        np.testing.assert_allclose(parts[0][0] + parts[1][0], whole, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(parts[0][1] + parts[1][1], tw, rtol=RTOL_SUM, atol=0)
        assert parts[0][1][14] + parts[1][1][14] == tw[14] > 0 and tw[11] > 0
        ctx.render_exitance(sc, h, 0, 32, seed=9)                              # accumulates onto the second half
        both, tb = ctx.exitance_fd_read(h)
        np.testing.assert_allclose(both, whole, rtol=RTOL_SUM, atol=0)
        assert tb[0] == PATHS and tb[14] == tw[14]
        _, t_only = ctx.exitance_fd_read(h, sums=False)
        assert np.array_equal(t_only, tb)
    finally:
        ctx.exitance_destroy(h)


def test_bounds_checking_build_reports_no_violation(ctx):
    """eight wavenumbers through libmer_check.so, cube and sphere, straight and curved: no index outside the 16 planes"""
    ks = (0.0, 0.3, 0.7, 1.1, 1.9, 3.0, 4.5, 7.0)
    cases = (TG.scattering(), TE._grid(rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=0.05, stepper=P.STEP_VERLET), TE._base(**TE._sphere()))
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for p in cases:
            got = []
            for cx in (c, ctx):
                sc, vols = cx.upload_scene(p, layout=capi.LAYOUT_DENSE)
                h = cx.exitance_fd_create(sc.boundary, (5, 3), ks, 0.1)
                cx.render_exitance(sc, h, 0, 8, seed=3)
                got.append(cx.exitance_fd_read(h))
                cx.exitance_destroy(h)
                for v in vols:
                    v.destroy()
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (n, kind, idx, lim)
            assert got[0][0].shape[:2] == (8, 2) and got[0][0].shape[3:] == (3, 5, 3) and np.abs(got[0][0][7]).sum() > 0
            scale = np.broadcast_to(got[1][0][:1, :1], got[1][0].shape)
            assert np.all(np.abs(got[0][0] - got[1][0]) <= RTOL_SUM * scale)
            np.testing.assert_allclose(got[0][1], got[1][1], rtol=RTOL_SUM, atol=0)
    finally:
        c.close()


def _create_refusals():
    """(desc, message) of every refusal of mer_exitance_fd_create"""
    def desc(boundary=P.BOUNDARY_AABB, res=(4, 4), k=KS, cos_min=0.0, reserved=0, tail=None, n_freq=None):
        d = capi.exitance_fd_desc(boundary, res, k, cos_min)
        d.reserved = reserved
        if tail is not None:
            d.wavenumber[7] = tail
        if n_freq is not None:
            d.n_freq = n_freq
        return d
    return ((desc(boundary=P.BOUNDARY_SDF), "boundary must be the cube"), (desc(res=(0, 4)), "res must lie in 1 ... 4096"),
            (desc(res=(4, 5000)), "res must lie in 1 ... 4096"), (desc(cos_min=1.0), "cos_min must lie in"), (desc(cos_min=-0.5), "cos_min must lie in"),
            (desc(n_freq=0), "n_freq must lie in 1 ... 8"), (desc(n_freq=9), "n_freq must lie in 1 ... 8"),
            (desc(k=(0.5, -1.0)), "a wavenumber must be finite and at least 0"), (desc(k=(float("inf"),)), "a wavenumber must be finite and at least 0"),
            (desc(tail=0.5), "the entries of wavenumber past n_freq must be 0"), (desc(reserved=3), "reserved must be 0"),
            (desc(res=(4096, 4096), k=(1.0,)), "more than 2\\^27 cells x faces x 2 x n_freq"))


def test_refusals(ctx):
    """every create refusal past the Python check, every read refusal, and a handle of the wrong family"""
    for d, msg in _create_refusals():
        out = C.c_int32(-1)
        assert ctx.lib.mer_exitance_fd_create(ctx.h, C.byref(d), C.byref(out)) != 0 and out.value == 0
        err = ctx.lib.mer_last_error(ctx.h).decode()
        assert err.startswith("mer_exitance_fd_create: ") and re.search(msg, err), err
    hs, hf = ctx.exitance_create(P.BOUNDARY_AABB, T.RES), ctx.exitance_fd_create(P.BOUNDARY_AABB, T.RES, KS)
    hg = ctx.fluence_fd_create((4, 4, 4), (-1, -1, -1), (1, 1, 1), KS)
    t16 = np.zeros(16)

    def read(fn, handle):
        assert getattr(ctx.lib, fn)(ctx.h, C.c_int32(handle), None, t16.ctypes.data_as(C.c_void_p)) != 0
        return ctx.lib.mer_last_error(ctx.h).decode()
    try:
        assert read("mer_exitance_read", hf) == "mer_exitance_read: frequency-domain map: use mer_exitance_fd_read"
        assert read("mer_exitance_fd_read", hs) == "mer_exitance_fd_read: steady or time-gated map: use mer_exitance_read"
        assert read("mer_exitance_fd_read", hg) == "mer_exitance_fd_read: unknown exitance handle"
        assert read("mer_exitance_fd_read", hf + 1000) == "mer_exitance_fd_read: unknown exitance handle"
        for call, handle, msg in ((ctx.exitance_read, hf, "mer_exitance_read: frequency-domain map: use mer_exitance_fd_read"),
                                  (ctx.exitance_fd_read, hs, "mer_exitance_fd_read: steady or time-gated map: use mer_exitance_read"),
                                  (ctx.exitance_fd_read, hg, "mer_exitance_fd_read: unknown exitance handle")):
            with pytest.raises(capi.MerError, match="^" + re.escape(msg) + "$"):
                call(handle)
        sc, _ = ctx.upload_scene(TG.scattering())
        with pytest.raises(capi.MerError, match="mer_render_exitance: unknown exitance handle"):
            ctx.render_exitance(sc, hg, 0, 1)
        with pytest.raises(capi.MerError, match="mer_exitance_destroy: unknown exitance handle"):
            ctx.exitance_destroy(hg)
        sph, _ = ctx.upload_scene(TE._base(**TE._sphere()))
        with pytest.raises(capi.MerError, match="the scene's boundary differs from the map's"):
            ctx.render_exitance(sph, hf, 0, 1)
        s, t = ctx.exitance_fd_read(hf)
        assert s.shape == (3, 2, 6, 4, 4, 3) and not s.any() and not t.any()
    finally:
        ctx.exitance_destroy(hs); ctx.exitance_destroy(hf); ctx.fluence_destroy(hg)


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def test_mer_render_frequencies_writes_the_python_calls_map(ctx, tmp_path):
    """mer_render --exitance=8,6 --frequencies=0,0.7 --accept-cos=0.25 on the laser example: the float32 .npy [n_freq][2][faces][nv][nu][3] =
    sums / (paths x cell area) of the map exitance_fd_read gives for the same scene and seed"""
    scene = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
    defines = {"samples": "2", "tMin": "4", "tMax": "9", "tRes": "0.5", "medium": "homogeneous"}
    out = str(tmp_path / "fd.npy")
    args = [os.path.join(ROOT, "mitsubaer_amd", "mer_render"), "--exitance=8,6", "--frequencies=0,0.7", "--accept-cos=0.25", "--seed", "3", "-o", out]
    for k, v in defines.items():
        args += ["-D", "%s=%s" % (k, v)]
    r = subprocess.run(args + [scene], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "paths %d " % (128 * 96 * 2) in r.stdout and "rejected" in r.stdout and "frequency 1  k 0.7" in r.stdout
    data = np.load(out)
    assert data.shape == (2, 2, 6, 6, 8, 3) and data.dtype == np.float32
    d, spp = host.flatten_xml(scene, defines)
    h = ctx.exitance_fd_create(d.boundary, (8, 6), (0.0, 0.7), 0.25)
    try:
        ctx.render_exitance(d, h, 0, spp, seed=3)
        sums, t = ctx.exitance_fd_read(h)
    finally:
        ctx.exitance_destroy(h)
    assert t[0] == 128 * 96 * 2 and sums[0, 0].sum() > 0 and t[11] > 0
    ext = np.array(d.bmax[:], np.float64) - np.array(d.bmin[:], np.float64)
    area = np.array([ext[(f // 2 + 1) % 3] * ext[(f // 2 + 2) % 3] / 48 for f in range(6)])
    want = sums / (t[0] * area[None, None, :, None, None, None])
    np.testing.assert_allclose(data, want.astype(np.float32), rtol=1e-6, atol=0)
    assert np.all(data[0, 1] == 0.0)
    amp, phase = [float(v) for v in re.search(r"frequency 1  k 0.7  amplitude (\S+)  phase (\S+)", r.stdout).groups()]
    re_, im_ = sums[1, 0].sum(), sums[1, 1].sum()
    np.testing.assert_allclose([amp, phase], [np.hypot(re_, im_), np.arctan2(im_, re_)], rtol=1e-6)
