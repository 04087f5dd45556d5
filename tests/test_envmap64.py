"""CPU self-checks of tests/envmap64.py, the float64 restatement of emitter `envmap` the GPU leaf tests are held to: pdfDirect integrates to
one over the sphere, sampleDirect draws directions with that density (chi-square), and its value / pdf is eval / pdfDirect at the direction it
returns -- on a power-of-two map, a non-power-of-two one and a tiny one, rotated, with the u seam and both poles."""
import numpy as np
import pytest
from scipy import stats
from tests.envmap64 import EnvMap64, sun_and_gradient, rot

MAPS = {"pow2": (16, 32), "npot": (24, 40), "tiny": (5, 3)}
R = rot([0.3, 1.0, -0.4], 57.0)


def _sphere_grid(nt=1200, nphi=2400):
    t = (np.arange(nt) + 0.5) * np.pi / nt
    ph = (np.arange(nphi) + 0.5) * 2 * np.pi / nphi
    T, PH = np.meshgrid(t, ph, indexing="ij")
    d = np.stack([np.sin(PH) * np.sin(T), np.cos(T), -np.cos(PH) * np.sin(T)], -1).reshape(-1, 3)
    return d, (np.sin(T) * (np.pi / nt) * (2 * np.pi / nphi)).reshape(-1)


@pytest.mark.parametrize("name", sorted(MAPS))
def test_pdf_integrates_to_one(name):
    m = EnvMap64(sun_and_gradient(*MAPS[name]), R)
    d, dw = _sphere_grid()
    assert abs((m.pdf(d @ R[:3, :3].T) * dw).sum() - 1.0) < 1e-3


@pytest.mark.parametrize("name", sorted(MAPS))
def test_sampling_matches_the_pdf(name):
    """chi-square of sampleDirect's directions in (theta, phi) bins of the map's frame against pdfDirect integrated over each bin"""
    m = EnvMap64(sun_and_gradient(*MAPS[name]), R)
    n, nt, nphi = 200000, 12, 24
    row, col, d, vop, pdf = m.sample(np.random.default_rng(7).random((n, 2)))
    _, _, v = m.uv(d)
    ti = np.minimum((np.arccos(np.clip(v[:, 1], -1, 1)) / np.pi * nt).astype(int), nt - 1)
    pi = np.minimum((np.mod(np.arctan2(v[:, 0], -v[:, 2]), 2 * np.pi) / (2 * np.pi) * nphi).astype(int), nphi - 1)
    obs = np.bincount(ti * nphi + pi, minlength=nt * nphi).astype(np.float64)
    g, dw = _sphere_grid(nt * 60, nphi * 60)
    p = m.pdf(g @ R[:3, :3].T) * dw
    exp = p.reshape(nt, 60, nphi, 60).sum((1, 3)).reshape(-1) * n
    keep = exp > 5
    assert exp[~keep].sum() < 1e-3 * n
    chi2 = (((obs - exp) ** 2 / exp)[keep]).sum()
    assert stats.chi2.sf(chi2, keep.sum() - 1) > 1e-3, chi2


@pytest.mark.parametrize("name", sorted(MAPS))
def test_value_over_pdf_is_eval_over_pdf(name):
    m = EnvMap64(sun_and_gradient(*MAPS[name]), R, scale=2.5)
    u2 = np.random.default_rng(8).random((20000, 2))
    u2[:8] = [[0.5, 0.0], [0.5, 1.0], [0.0, 0.5], [1.0, 0.5], [0.25, 1e-9], [0.75, 1 - 1e-9], [1e-9, 0.3], [1 - 1e-9, 0.6]]    # poles, the seam
    row, col, d, vop, pdf = m.sample(u2)
    val, p = m.eval(d)
    # within half a texel row of a pole the tent offset can cross it: the sample then blends the texels on its own side of the pole while
    # the look-up of the direction it returns sees the other side (the reference does the same: envmap.cpp:567-608)
    _, _, v = m.uv(d)
    ok = (pdf > 1e-6 * pdf.max()) & (np.abs(v[:, 1]) < np.cos(0.5 * np.pi / m.h))
    assert ok.mean() > 0.9
    np.testing.assert_allclose(pdf[ok], p[ok], rtol=1e-6)
    np.testing.assert_allclose(vop[ok], val[ok] / p[ok, None], rtol=1e-6)


def test_seam_is_continuous_and_poles_clamp():
    """u wraps at +-1/2 (ERepeat): the look-up is continuous across the seam; v clamps (EClamp): at a pole the look-up is the first / last
    texel row, interpolated in u"""
    img = sun_and_gradient(24, 40)
    m = EnvMap64(img)
    t = np.linspace(0.1, 3.0, 50)
    a = np.stack([np.full_like(t, 1e-9), np.cos(t), np.sin(t)], 1)
    b = np.stack([np.full_like(t, -1e-9), np.cos(t), np.sin(t)], 1)
    np.testing.assert_allclose(m.eval(a)[0], m.eval(b)[0], rtol=1e-6)
    # at the +y pole with phi = 2 pi (x + 0.5) / W, the look-up is texel (x, 0)
    x = np.arange(40)
    phi = 2 * np.pi * (x + 0.5) / 40
    near = np.stack([1e-9 * np.sin(phi), np.ones_like(phi), -1e-9 * np.cos(phi)], 1)
    np.testing.assert_allclose(m.eval(near)[0], m.tex[0, x], rtol=1e-5)
    np.testing.assert_allclose(m.eval(near * [1, -1, 1])[0], m.tex[-1, x], rtol=1e-5)


def test_tables_follow_configure():
    """the CDF rows end at 1, the texels are half-rounded, and the black / non-finite maps are refused with the reference's messages"""
    img = sun_and_gradient(24, 40)
    m = EnvMap64(img)
    assert m.cdf_rows[0] == 0 and m.cdf_rows[-1] == 1 and (m.cdf_cols[:, -1] == 1).all() and (np.diff(m.cdf_rows) >= 0).all()
    assert (m.tex == img.astype(np.float16).astype(np.float64)).all()
    with pytest.raises(ValueError, match="completely black"):
        EnvMap64(np.zeros((4, 8, 3)))
    with pytest.raises(ValueError, match="nan/inf"):
        EnvMap64(np.full((4, 8, 3), 1e6))
