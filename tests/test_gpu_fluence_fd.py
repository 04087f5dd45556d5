"""Frequency-domain fluence grids (mer_fluence_fd_create, the FD kind of K_fluence) on the GPU: the complex Beer-Lambert column of a pure
absorber, same-seed identities against the steady and the time-resolved grid on one scene per kind of instantiation, the float64 restatement
tests/fd64.py in a scattering and in a chromatic medium, and the interface: shards, clear / accumulate, the bounds-checking build, the
refusals, `mer_render --fluence --frequencies`.

Set-up (tests/test_exitance64.py, tests/test_fd64.py): a 16 x 16 film (path enumeration only) x 64 samples = 16 384 paths per batch, K = 16
batches with seeds s0 + j, the beam of power 5 from (0.2, 0.1, -3) along +z into the cube, wavenumbers (0, 0.7, 3.0),
medium_sampling_weight = 1.  The bar is the project's; a value is left out of a comparison only when it is exactly 0.0 in every batch on both
sides.

Measured on an MI355X (this file's seeds): the column 0 of 40 values beyond 4 sigma (largest z 1.77, n = 1; 1.76, n = 1.4); the identities:
modulus / steady at most 1.000000000, DFT difference at most 0.997 of the bound (bspline); against float64: 0 of 320 (2.77), chromatic 0 of
960 (3.58)."""
import ctypes as C
import os
import re
import subprocess
import numpy as np
import pytest
from mitsubaer_amd import params as P, capi, host
from tests import test_fd64 as TF
from tests import test_gpu_exitance as TE
from tests import test_gpu_lightpath_parent as TL

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K, PATHS, SPP, RTOL_SUM = TE.K, TE.PATHS, TE.SPP, TE.RTOL_SUM
KS = TF.KS
CUBE = ((-1, -1, -1), (1, 1, 1))
T_BIN = 0.05                                   # of the timed handle the phases are held to
COUNTERS = TL.COUNTERS


def absorber(n):
    return TE._base(sigma_s=[0.0] * 3, sigma_a=[TF.ABSORBER] * 3, g=0.0, rif_const=n)


def scattering():
    return TE._base(sigma_s=[TF.SIGMA_S] * 3, sigma_a=[TF.SIGMA_A] * 3, g=TF.G, rif_const=TF.N)


def chromatic():
    return TE._base(sigma_s=list(TF.CHROMA_S), sigma_a=list(TF.CHROMA_A), g=TF.G, rif_const=TF.N, strategy=P.STRATEGY_SINGLE)


def _batches(ctx, p, seed0, res, ks=KS, k=K):
    """k batches with seeds seed0 + j into one grid, cleared in between: raw sums (k, n_freq, 2, nz, ny, nx, 3), totals (k, 8)"""
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    h = ctx.fluence_fd_create(res, *CUBE, ks)
    sums, totals = [], []
    try:
        for j in range(k):
            ctx.fluence_clear(h)
            ctx.render_fluence(sc, h, 0, SPP, seed=seed0 + j)
            s, t = ctx.fluence_fd_read(h)
            assert np.isfinite(s).all() and np.isfinite(t).all()
            sums.append(s); totals.append(t)
    finally:
        ctx.fluence_destroy(h)
        for v in vols:
            v.destroy()
    return np.array(sums), np.array(totals)


def grey(sums):
    """a grey scene: the three channels hold the same sums, added in their own order.  A plane's deposits change sign, so the channels are
    held together by the size of the cell's steady sum -- the real plane of k = 0, KS[0] -- times RTOL_SUM; returns channel 0"""
    assert KS[0] == 0.0
    scale = RTOL_SUM * sums[:, :1, :1, ..., 0]
    assert np.all(np.abs(sums[..., 1] - sums[..., 0]) <= scale) and np.all(np.abs(sums[..., 2] - sums[..., 0]) <= scale)
    return sums[..., 0]


# ---- 3. the absorber's column ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", [1.0, 1.4])
def test_absorber_column_holds_the_complex_beer_lambert_law(ctx, n):
    """the column cell over the depths [a, b] holds PATHS P e^{2 i k} (e^{c b} - e^{c a}) / c, c = -sigma_a + i k n, in both planes of every
    wavenumber; every cell off the column and the imaginary plane of k = 0 are exactly 0"""
    sums, tot = _batches(ctx, absorber(n), 2100, TF.COLUMN_RES)
    g = grey(sums)
    assert g.shape == (K, 3, 2, 8, 4, 4)
    zmax = TF.check_column(g, n, "GPU, n %.1f" % n)
    print("n %.1f: column max z %.2f" % (n, zmax))
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 4:8] == 0)


# ---- 5. same-seed identities -------------------------------------------------------------------------------------------------------------

MAX_DEPTH = 6


def bounded(name):
    """the scene of tests/test_gpu_lightpath_parent.py with a max_depth that bounds the path length, and that bound: the exterior leg (at most
    the beam's 2 units ... the far corner's 2 sqrt 27) and per depth one flight across the cube (2 sqrt 3; a curved ray's arc may be longer
    than the chord: x 1.25) at an index of at most 1.6 (the largest of the fields: 1.45).  The timed handle checks the bound: nothing may fall out of its window"""
    p = TL.SCENES[name]()
    if p.max_depth < 0 or p.max_depth > MAX_DEPTH:
        p.max_depth = MAX_DEPTH
    return p, 2.0 + p.max_depth * 2.0 * np.sqrt(3.0) * 1.25 * 1.6


def dft_of_frames(timed, ks, t_min=0.0, t_bin=T_BIN):
    """sum_f timed[f] e^{i k centre_f}: (n_freq, 2, ...) from (frames, ...)"""
    centre = t_min + (np.arange(timed.shape[0]) + 0.5) * t_bin
    out = np.zeros((len(ks), 2) + timed.shape[1:])
    for j, k in enumerate(ks):
        out[j, 0] = np.tensordot(np.cos(k * centre), timed, 1)
        out[j, 1] = np.tensordot(np.sin(k * centre), timed, 1)
    return out


def check_identities(fd, steady, timed, ks, l_max, what):
    """checks 2 - 4 of the same-seed identities: fd (n_freq, 2, cells..., 3), steady (cells..., 3), timed (frames, cells..., 3); returns the
    largest (DFT difference / bound) and (modulus / steady)"""
    np.testing.assert_allclose(fd[0, 0], steady, rtol=RTOL_SUM, atol=0, err_msg=what + ": the real plane of k = 0")
    assert np.all(fd[0, 1] == 0.0), what + ": the imaginary plane of k = 0"
    np.testing.assert_allclose(timed.sum(0), steady, rtol=RTOL_SUM, atol=0, err_msg=what + ": the window holds every deposit")
    mod = np.hypot(fd[:, 0], fd[:, 1])
    assert np.all(mod <= steady[None] * (1 + RTOL_SUM)), what + ": a modulus above the steady sum"
    dft = dft_of_frames(timed, ks)
    worst = 0.0
    for j, k in enumerate(ks):
        bound = k * (T_BIN / 2 + 2.0 ** -22 * l_max) * steady + 1e-9 * steady
        diff = np.hypot(fd[j, 0] - dft[j, 0], fd[j, 1] - dft[j, 1])
        assert np.all(diff <= bound), (what, k, float((diff / np.maximum(bound, 1e-300)).max()))
        if k > 0 and np.any(steady > 0):
            worst = max(worst, float((diff[steady > 0] / bound[steady > 0]).max()))
    filled = steady > 0
    return worst, float((mod[:, filled] / steady[None][:, filled]).max()) if filled.any() else 0.0


def counted(ctx, render):
    ctx.counters_reset()
    render()
    cnt = ctx.counters()
    return [int(cnt[q]) for q in COUNTERS]


@pytest.mark.parametrize("name", sorted(TL.SCENES))
def test_same_seed_identities(ctx, name):
    """one scene per kind of instantiation, 1024 paths, an 8^3 box: the frequency-domain handle against the steady and the timed handle of
    the same scene, shard and seed -- the same walk (counters, paths, ended), the steady grid in the real plane of k = 0, a modulus never
    above the steady sum, and the phase within half a bin of the timed grid's: this pins the phase on curved rays to the path length the
    timed recorders pin against a float64 eikonal trace"""
    p, l_max = bounded(name)
    frames = int(np.ceil(l_max / T_BIN))
    assert 512 * frames <= 1 << 27
    sc, vols = ctx.upload_scene(p, layout=capi.LAYOUT_DENSE)
    hs, ht, hf = ctx.fluence_create(*TL.BOX), ctx.fluence_time_create(*TL.BOX, frames=frames, t_min=0.0, t_bin=T_BIN), ctx.fluence_fd_create(*TL.BOX, KS)
    try:
        cs = counted(ctx, lambda: ctx.render_fluence(sc, hs, 0, TL.SPP, seed=TL.SEED))
        ct = counted(ctx, lambda: ctx.render_fluence(sc, ht, 0, TL.SPP, seed=TL.SEED))
        cf = counted(ctx, lambda: ctx.render_fluence(sc, hf, 0, TL.SPP, seed=TL.SEED))
        (steady, ts), (timed, tt), (fd, tf) = ctx.fluence_read(hs), ctx.fluence_time_read(ht), ctx.fluence_fd_read(hf)
    finally:
        for h in (hs, ht, hf):
            ctx.fluence_destroy(h)
        for v in vols:
            v.destroy()
    print(name, "counters", cf, "totals", list(tf))
    assert cf == cs == ct and cf[0] == TL.PATHS
    assert tf[0] == ts[0] == TL.PATHS and tf[7] == ts[7]
    np.testing.assert_allclose(tf, ts, rtol=RTOL_SUM, atol=0)
    assert np.all(tt[8:11] == 0), "deposits outside the timed window: the bound on the path length does not hold"
    if name != "beam_misses":
        assert steady.sum() > 0 and np.abs(fd[1:, 1]).sum() > 0
    worst, mod = check_identities(fd, steady, timed, KS, frames * T_BIN, name)
    print("%s: largest DFT difference / bound %.3f, largest modulus / steady %.9f" % (name, worst, mod))


# ---- 7. against the float64 restatement --------------------------------------------------------------------------------------------------

def test_scattering_medium_matches_float64(ctx):
    """sigma_s 2, sigma_a 0.1, g 0.8, n 1.4 on a 4^3 grid: every value of both planes under the bar"""
    r = TF.scattering_ref()
    sums, tot = _batches(ctx, scattering(), 2300, TF.GRID_RES)
    g = grey(sums)[..., None]
    assert g.shape == r["grid"].shape
    n, zmax = TF.compare(g, tot, r["grid"], r["grid_totals"], "GPU grid", (1,))
    print("scattering grid: %d values compared, max z %.2f" % (n, zmax))
    assert n == 384 - 64 and np.all(g[:, 0, 1] == 0.0)
    assert np.all(tot[:, 0] == PATHS) and np.all(tot[:, 7] == 0) and np.all(tot[:, 4:7] == 0)


def test_chromatic_medium_matches_float64(ctx):
    """three different sigma_t under strategy single: the deposit is tau_c / pdfSuccess per channel"""
    r = TF.chromatic_ref()
    sums, tot = _batches(ctx, chromatic(), 2400, TF.GRID_RES)
    assert sums.shape == r["grid"].shape
    n, zmax = TF.compare(sums, tot, r["grid"], r["grid_totals"], "GPU chromatic grid", (1, 2, 3))
    print("chromatic grid: %d values compared, max z %.2f" % (n, zmax))
    assert n == 3 * (384 - 64)
    col = sums[:, 0, 0].sum(0).reshape(-1, 3).sum(0)
    assert not np.isclose(col[0], col[1], rtol=1e-3) and not np.isclose(col[1], col[2], rtol=1e-3)


# ---- 8. the interface --------------------------------------------------------------------------------------------------------------------

def test_half_shards_add_up_and_the_grid_accumulates(ctx):
    sc, _ = ctx.upload_scene(scattering())
    h = ctx.fluence_fd_create(TF.GRID_RES, *CUBE, KS)
    try:
        ctx.render_fluence(sc, h, 0, SPP, seed=9)
        whole, tw = ctx.fluence_fd_read(h)
        parts = []
        for begin in (0, 32):
            ctx.fluence_clear(h)
            z, tz = ctx.fluence_fd_read(h)
            assert not z.any() and not tz.any()
            ctx.render_fluence(sc, h, begin, 32, seed=9)
            parts.append(ctx.fluence_fd_read(h))
        assert parts[0][1][0] == parts[1][1][0] == PATHS // 2 and tw[0] == PATHS
        assert np.abs(parts[0][0]).sum() > 0 and not np.array_equal(parts[0][0], parts[1][0])
        np.testing.assert_allclose(parts[0][0] + parts[1][0], whole, rtol=RTOL_SUM, atol=0)
        np.testing.assert_allclose(parts[0][1] + parts[1][1], tw, rtol=RTOL_SUM, atol=0)
        ctx.render_fluence(sc, h, 0, 32, seed=9)                               # accumulates onto the second half
        both, tb = ctx.fluence_fd_read(h)
        np.testing.assert_allclose(both, whole, rtol=RTOL_SUM, atol=0)
        assert tb[0] == PATHS
        _, t_only = ctx.fluence_fd_read(h, sums=False)
        assert np.array_equal(t_only, tb)
    finally:
        ctx.fluence_destroy(h)


def test_bounds_checking_build_reports_no_violation(ctx):
    """eight wavenumbers through libmer_check.so, straight and curved: no index outside the 16 planes, and the sums of the plain build"""
    ks = (0.0, 0.3, 0.7, 1.1, 1.9, 3.0, 4.5, 7.0)
    cases = (scattering(), TE._grid(rif_mode=P.RIF_TRILINEAR, rif=TE._rif(), stepsize=0.05, stepper=P.STEP_VERLET))
    c = capi.Context(0, check=True)
    try:
        assert c.debug_bounds()[0]
        for p in cases:
            got = []
            for cx in (c, ctx):
                sc, vols = cx.upload_scene(p, layout=capi.LAYOUT_DENSE)
                h = cx.fluence_fd_create((5, 3, 4), *CUBE, ks)
                cx.render_fluence(sc, h, 0, 8, seed=3)
                got.append(cx.fluence_fd_read(h))
                cx.fluence_destroy(h)
                for v in vols:
                    v.destroy()
            en, n, kind, idx, lim = c.debug_bounds()
            assert n == 0, (n, kind, idx, lim)
            assert got[0][0].shape == (8, 2, 4, 3, 5, 3) and np.abs(got[0][0][7]).sum() > 0
            scale = np.broadcast_to(got[1][0][:1, :1], got[1][0].shape)
            assert np.all(np.abs(got[0][0] - got[1][0]) <= RTOL_SUM * scale)
            np.testing.assert_allclose(got[0][1], got[1][1], rtol=RTOL_SUM, atol=0)
    finally:
        c.close()


def test_refusals(ctx):
    """every create refusal past the Python check, every read refusal, and a handle of the wrong family"""
    for d, msg in _create_refusals():
        out = C.c_int32(-1)
        assert ctx.lib.mer_fluence_fd_create(ctx.h, C.byref(d), C.byref(out)) != 0 and out.value == 0
        err = ctx.lib.mer_last_error(ctx.h).decode()
        assert err.startswith("mer_fluence_fd_create: ") and re.search(msg, err), err
    hs, ht, hf = ctx.fluence_create((4, 4, 4), *CUBE), ctx.fluence_time_create((4, 4, 4), *CUBE, frames=2, t_min=0.0, t_bin=1.0), ctx.fluence_fd_create((4, 4, 4), *CUBE, KS)
    he = ctx.exitance_fd_create(P.BOUNDARY_AABB, (4, 4), KS)
    t16 = np.zeros(16)

    def read(fn, handle):
        assert getattr(ctx.lib, fn)(ctx.h, C.c_int32(handle), None, t16.ctypes.data_as(C.c_void_p)) != 0
        return ctx.lib.mer_last_error(ctx.h).decode()
    try:
        assert read("mer_fluence_read", hf) == "mer_fluence_read: frequency-domain grid: use mer_fluence_fd_read"
        assert read("mer_fluence_time_read", hf) == "mer_fluence_time_read: frequency-domain grid: use mer_fluence_fd_read"
        assert read("mer_fluence_fd_read", hs) == "mer_fluence_fd_read: steady-state grid: use mer_fluence_read"
        assert read("mer_fluence_fd_read", ht) == "mer_fluence_fd_read: time-resolved grid: use mer_fluence_time_read"
        assert read("mer_fluence_fd_read", he) == "mer_fluence_fd_read: unknown fluence handle"
        assert read("mer_fluence_fd_read", hf + 1000) == "mer_fluence_fd_read: unknown fluence handle"
        # the Python front end says the same before it sizes the array
        for call, handle, msg in ((ctx.fluence_read, hf, "mer_fluence_read: frequency-domain grid: use mer_fluence_fd_read"),
                                  (ctx.fluence_time_read, hf, "mer_fluence_time_read: frequency-domain grid: use mer_fluence_fd_read"),
                                  (ctx.fluence_fd_read, hs, "mer_fluence_fd_read: steady-state grid: use mer_fluence_read"),
                                  (ctx.fluence_fd_read, ht, "mer_fluence_fd_read: time-resolved grid: use mer_fluence_time_read"),
                                  (ctx.fluence_fd_read, he, "mer_fluence_fd_read: unknown fluence handle")):
            with pytest.raises(capi.MerError, match="^" + re.escape(msg) + "$"):
                call(handle)
        sc, _ = ctx.upload_scene(scattering())
        with pytest.raises(capi.MerError, match="mer_render_fluence: unknown fluence handle"):
            ctx.render_fluence(sc, he, 0, 1)
        with pytest.raises(capi.MerError, match="mer_fluence_clear: unknown fluence handle"):
            ctx.fluence_clear(he)
        sc.integrator = P.INTEGRATOR_VOLPATH
        with pytest.raises(capi.MerError, match="mer_render_fluence: the scene's integrator must be ptracer"):
            ctx.render_fluence(sc, hf, 0, 1)
        s, t = ctx.fluence_fd_read(hf)
        assert s.shape == (3, 2, 4, 4, 4, 3) and not s.any() and not t.any()
    finally:
        for h in (hs, ht, hf):
            ctx.fluence_destroy(h)
        ctx.exitance_destroy(he)


def _create_refusals():
    """(desc, message) of every refusal of mer_fluence_fd_create"""
    def desc(res=(4, 4, 4), bmin=CUBE[0], bmax=CUBE[1], k=KS, reserved=(0, 0), tail=None, n_freq=None):
        d = capi.fluence_fd_desc(res, bmin, bmax, k)
        d.reserved[:] = reserved
        if tail is not None:
            d.wavenumber[7] = tail
        if n_freq is not None:
            d.n_freq = n_freq
        return d
    return ((desc(res=(0, 4, 4)), "res must lie in 1 ... 1024"), (desc(bmin=(-1, float("inf"), -1)), "bmin / bmax must be finite"),
            (desc(bmin=(1, -1, -1)), "bmin must be below bmax"), (desc(res=(1024, 1024, 1024)), "more than 2\\^27 cells$"),
            (desc(n_freq=0), "n_freq must lie in 1 ... 8"), (desc(n_freq=9), "n_freq must lie in 1 ... 8"),
            (desc(k=(0.5, -1.0)), "a wavenumber must be finite and at least 0"), (desc(k=(float("nan"),)), "a wavenumber must be finite and at least 0"),
            (desc(tail=0.5), "the entries of wavenumber past n_freq must be 0"), (desc(reserved=(0, 7)), "reserved must be 0"),
            (desc(res=(512, 512, 512), k=(1.0,)), "more than 2\\^27 cells x 2 x n_freq"))


# ---- the command line --------------------------------------------------------------------------------------------------------------------

def test_mer_render_frequencies_writes_the_python_calls_grid(ctx, tmp_path):
    """mer_render --fluence=4,4,4 --frequencies=0,0.7 on the laser example: the float32 .npy [n_freq][2][nz][ny][nx][3] = sums / (paths x cell
    volume) of the grid fluence_fd_read gives for the same scene and seed, and the printed amplitude and phase of the summed planes"""
    scene = os.path.join(ROOT, "scenes", "cfg_laser_transient.xml")
    defines = {"samples": "2", "tMin": "4", "tMax": "9", "tRes": "0.5", "medium": "homogeneous"}
    out = str(tmp_path / "fd.npy")
    args = [os.path.join(ROOT, "mitsubaer_amd", "mer_render"), "--fluence=4,4,4", "--frequencies=0,0.7", "--seed", "3", "-o", out]
    for k, v in defines.items():
        args += ["-D", "%s=%s" % (k, v)]
    r = subprocess.run(args + [scene], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert "paths %d " % (128 * 96 * 2) in r.stdout and "frequency 1  k 0.7" in r.stdout
    data = np.load(out)
    assert data.shape == (2, 2, 4, 4, 4, 3) and data.dtype == np.float32
    d, spp = host.flatten_xml(scene, defines)
    bmin, bmax = np.array(d.bmin[:], np.float64), np.array(d.bmax[:], np.float64)
    h = ctx.fluence_fd_create((4, 4, 4), d.bmin[:], d.bmax[:], (0.0, 0.7))
    try:
        ctx.render_fluence(d, h, 0, spp, seed=3)
        sums, t = ctx.fluence_fd_read(h)
    finally:
        ctx.fluence_destroy(h)
    assert t[0] == 128 * 96 * 2 and sums[0, 0].sum() > 0
    want = sums / (t[0] * np.prod((bmax - bmin) / 4))
    np.testing.assert_allclose(data, want.astype(np.float32), rtol=1e-6, atol=0)      # float32 rounding (the float64 atomics' order is far below it)
    assert np.all(data[0, 1] == 0.0)
    amp, phase = [float(v) for v in re.search(r"frequency 1  k 0.7  amplitude (\S+)  phase (\S+)", r.stdout).groups()]
    re_, im_ = sums[1, 0].sum(), sums[1, 1].sum()
    np.testing.assert_allclose([amp, phase], [np.hypot(re_, im_), np.arctan2(im_, re_)], rtol=1e-6)
