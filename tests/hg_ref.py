"""Shared float64 checks of a Henyey-Greenstein sampler / evaluator pair (the oracle's and the HIP kernels'): tests/ref64.py is the
ground truth, numpy only.  Used by tests/test_ref64.py and tests/test_gpu_closed_form.py."""
import numpy as np
from tests import ref64

EPS32 = 2.0 ** -24
HG_EPSILON = 1e-4          # below |g| = Epsilon hg.cpp samples cos theta = 1 - 2u
G_EDGES = [0.999, -0.999, 0.99, -0.99, 2e-4, -2e-4, 1.01e-4, 9.9e-5]
# |wo| - 1: for 1e-4 < |g| < ~2e-4 the float32 cos theta = (1 + g^2 - sq^2) / 2g cancels and can round above 1; safe_sqrt then gives
# sin theta = 0 and wo = cos theta * frame normal, |wo| = cos theta (measured 1.7e-5 in the oracle).  The reference's sampler has the same form.
WO_SLACK = 2e-5


def _chi2_crit(df, z=3.719):
    """Wilson-Hilferty upper quantile of chi^2(df); z = 3.719 is the standard normal's 1e-4 upper quantile"""
    return df * (1 - 2.0 / (9 * df) + z * np.sqrt(2.0 / (9 * df))) ** 3


def mu_tolerance(g, u):
    """bound on the float32 error of cos theta = (1 + g^2 - sq^2) / 2g, sq = (1 - g^2) / (1 - g + 2 g u): propagate a relative rounding
    of a few ulp through each operation; the denominator 1 - g + 2gu cancels as u -> 1 for g -> -1"""
    u = np.asarray(u, np.float64)
    if abs(g) < HG_EPSILON:
        return np.full(u.shape, 8 * EPS32)
    den = 1 - g + 2 * g * u
    sq = (1 - g * g) / den
    rel_sq = 4 * EPS32 * (1 + (1 + g * g) / (1 - g * g) + (abs(1 - g) + 2 * abs(g) * u) / np.abs(den))      # 1 - g^2 cancels too
    return 8 * EPS32 * (1 + g * g + 2 * sq * sq * (1 + rel_sq / EPS32)) / (2 * abs(g)) + 8 * EPS32


def check_hg(sample, evaluate, g, n=200000, seed=0):
    """sample(wi, u2) -> (wo, pdf); evaluate(wi, wo) -> pdf.  Returns a dict of the largest errors seen (asserted here)."""
    g = float(np.float32(g))
    rng = np.random.RandomState(seed)
    v = rng.normal(size=(n, 3)); wi = (v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    u2 = rng.rand(n, 2).astype(np.float32)
    wo, pdf = sample(wi, u2)
    assert np.isfinite(wo).all() and np.isfinite(pdf).all()
    wo64 = wo.astype(np.float64); wi64 = wi.astype(np.float64)
    norm_err = np.abs(np.linalg.norm(wo64, axis=1) - 1).max()
    assert norm_err < WO_SLACK, norm_err
    mu = -(wi64 * wo64).sum(1) / np.linalg.norm(wo64, axis=1)
    # per sample: cos theta is the float64 inverse CDF of the first uniform number
    u = u2[:, 0].astype(np.float64)
    mu64 = 1 - 2 * u if abs(g) < HG_EPSILON else ref64.hg_inverse_cdf(g, u)
    mu_err = np.abs(mu - mu64)
    assert (mu_err <= mu_tolerance(g, u)).all(), ((mu_err / mu_tolerance(g, u)).max(), g)
    # chi^2 of cos theta against the float64 CDF: 50 equiprobable bins, merged where narrower than 1e-4 (a strongly peaked lobe puts
    # equiprobable edges closer together than the float32 resolution of cos theta near +-1)
    B = 50
    cand = ref64.hg_inverse_cdf(g, np.arange(1, B) / B) if abs(g) >= HG_EPSILON else 2 * np.arange(1, B) / B - 1
    edges = [-1.0]
    for e in cand:
        if e - edges[-1] >= 1e-4 and 1.0 - e >= 1e-4:
            edges.append(float(e))
    edges = np.array(edges[1:])
    cdf = np.concatenate([[0.0], ref64.hg_cdf(g, edges) if abs(g) >= HG_EPSILON else 0.5 * (edges + 1), [1.0]])
    expect = n * np.diff(cdf)
    cnt = np.bincount(np.searchsorted(edges, mu), minlength=len(expect))
    assert expect.min() > 5 and len(expect) >= 4, (len(expect), expect.min())
    chi2 = ((cnt - expect) ** 2 / expect).sum()
    assert chi2 < _chi2_crit(len(expect) - 1), (chi2, len(expect), g)
    # mean cosine = g within 4 sigma; E[cos^2] = (1 + 2 g^2) / 3
    sd = np.sqrt(((1 + 2 * g * g) / 3 - g * g) / n)
    assert abs(mu.mean() - g) < 4 * sd, (mu.mean(), g, sd)
    # pdf against float64 at the sampled direction: relative error scales with the conditioning (1 + g^2) / (1 + g^2 - 2 g cos)
    cosw = -(wi64 * wo64).sum(1)
    p64 = ref64.hg_pdf(g, cosw)
    rel = np.abs(pdf / p64 - 1)
    cond = ref64.hg_condition(g, cosw)
    assert (rel <= 4e-5 * cond + 1e-6).all(), ((rel / cond).max(), g)
    ev = evaluate(wi, wo)
    rel_ev = np.abs(ev / p64 - 1)
    assert (rel_ev <= 4e-5 * cond + 1e-6).all(), ((rel_ev / cond).max(), g)
    return dict(mu=float(mu_err.max()), norm=float(norm_err), pdf_over_cond=float((rel / cond).max()), chi2=float(chi2))
