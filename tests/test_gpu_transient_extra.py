"""Decomposed films -- transient, bounce, modulated -- of the scenes only the EXTRA / AREA kernels render, against the float64 references of
tests/transient64.py (checked on the CPU by tests/test_transient64.py): every site at which K_gen and K_event attach a path length to a
contribution that the oracle does not know -- the area luminaire sample, the look-up that ends on a shape, the unscattered escape, the
directly viewed shape, the map's sample and look-up, the camera edge of the lens and parallel sensors, calibrated_transient and the bounce
rule at each of them.  The GPU renders 32 batches; variances come from the batches and from the reference's own samples.

a. single scattering through the pencil camera, one emitter, per frame against a quadrature (frames [2, 10) of 0.25);
b. multiple scattering, transient [0, 16) of 0.5, per cell (a frame of a 4 x 4 pixel block) and per frame total;
c. the same as a bounce film, max_depth 8;
d. modulated films per pixel, the float64 walk weighted by the oracle's correlation function (pinned by tests/test_oracle_kat.py);
e. in b and c the GPU film must also DISAGREE with the float64 film of a wrong bookkeeping (tests/transient64.py: `wrong`).

Exactly one scattering vertex is max_depth 3 for the spot (inside the cube) and 4 for the emitters outside it: the null crossing of a
connection costs a depth of its own (include/mer.h), so at max_depth 3 nothing outside the cube reaches the one vertex.

Which cells and frame totals are tested is decided on the reference alone (transient64.tested_cells): those whose standard error in the
reference is below 25 % of their mean; the others are pooled with the next frame.  The multiple-scattering films (b, c) render batches of
transient64.MULTI_BATCH samples, not 64: see there."""
import numpy as np
import pytest
from tests import transient64 as T

pytestmark = pytest.mark.gpu


def _batches(ctx, p, B=32, spp=64, seed=11):
    """B independent renders of S samples, as tests/test_gpu_sensors._stats: the red channel of every frame, [B, H, W, F]"""
    sc, vols = ctx.upload_scene(p)
    x = []
    for b in range(B):
        f = ctx.render_to_host(sc, b * spp, spp, seed=seed).astype(np.float64)
        x.append(f[..., :-2].reshape(f.shape[0], f.shape[1], -1, 3)[..., 0] / f[..., -1:])
    for v in vols:
        v.destroy()
    return T.Batches(np.stack(x))


# ---- a. single-scatter profiles

@pytest.mark.parametrize("name", T.SINGLE_NAMES)
def test_single_scatter_profile_matches_the_quadrature(ctx, name):
    """plain and calibrated: the calibrated profile is the plain one 8 frames earlier"""
    F = T.SINGLE_FRAMES[2]
    wide = T.single_profile(name)
    for calibrated, prof in ((False, wide[:F]), (True, wide[8:])):
        g = _batches(ctx, T.single_params(name, calibrated_transient=calibrated))
        tot = g.totals.mean(0); cov = np.cov(g.totals.T) / g.B
        z = T.profile_z(tot, cov, prof)
        print("%s%s: max |z| %.2f over %d pools, totals %.5f vs %.5f" % (name, " calibrated" if calibrated else "", np.abs(z).max(), len(z), tot.sum(), prof.sum()))
        assert prof.sum() > 0 and len(z) >= 4 and len(z) >= 0.75 * T.resolved_frames(prof)     # pooling only gathers the frames the support grazes
        assert np.all(np.abs(z) <= 4), z
        assert np.all(g.totals[:, prof == 0] == 0)                                # frames the quadrature leaves empty hold exactly nothing


# ---- b. / e. multiple scattering, transient

def _judge(gpu, right, wrong):
    groups = T.tested(right)
    ok = T.compare(gpu, right, groups)
    bad = T.compare(gpu, wrong, groups)
    assert ok[0], ok
    assert not bad[0], bad


@pytest.mark.parametrize("name", T.MULTI_NAMES)
def test_transient_film_matches_float64(ctx, name):
    p, _ = T.multi_scene(name)
    R = T.multi_reference(name)
    _judge(_batches(ctx, T.decomposed(p, "transient"), spp=T.MULTI_BATCH), R["transient"], R["transient/edge_from_exit"])


@pytest.mark.parametrize("name", T.LENS_NAMES)
def test_calibrated_transient_film_matches_float64(ctx, name):
    """the edge dropped depends on the aperture sample; the wrong film is the one that keeps it"""
    p, _ = T.multi_scene(name)
    R = T.multi_reference(name)
    _judge(_batches(ctx, T.decomposed(p, "calibrated"), spp=T.MULTI_BATCH), R["calibrated"], R["transient"])


# ---- c. / e. bounce

@pytest.mark.parametrize("name", T.MULTI_NAMES)
def test_bounce_film_matches_float64(ctx, name):
    p, _ = T.multi_scene(name)
    R = T.multi_reference(name)
    _judge(_batches(ctx, T.decomposed(p, "bounce"), spp=T.MULTI_BATCH), R["bounce"], R["bounce/bounce_counts_exit"])


def test_calibrated_transient_does_not_reach_a_bounce_film(ctx):
    """the same film on the same streams, to the order of the film's atomic adds (the bound of tests/test_gpu_transient.py); a flag that leaked
    would move every contribution one frame down"""
    p, _ = T.multi_scene("lens_map_spot_point_rect")
    films = []
    for flag in (False, True):
        sc, _ = ctx.upload_scene(T.decomposed(p, "bounce", calibrated_transient=flag))
        films.append(ctx.render_to_host(sc, 0, 64, seed=11))
    assert films[0][..., :-2].sum() > 0
    np.testing.assert_allclose(films[0], films[1], rtol=1e-5, atol=1e-6)


# ---- d. modulated

@pytest.mark.parametrize("what", ["sine", "square"])
@pytest.mark.parametrize("name", T.MODULATED_NAMES)
def test_modulated_film_matches_float64(ctx, name, what):
    p, _ = T.multi_scene(name)
    R = T.multi_reference(name)
    q = T.decomposed(p, what)
    sc, _ = ctx.upload_scene(q)
    assert ctx.film_channels(sc) == 5
    gpu = _batches(ctx, q)
    ok = T.agrees_per_pixel(gpu, R[what])
    bad = T.agrees_per_pixel(gpu, R["square" if what == "sine" else "sine"])
    assert ok[0], ok
    assert not bad[0], bad
