"""The rough dielectric boundary (hroughdielectric) without a GPU: XML vocabulary and its refusals (C++ host and capi's validation), the
scene-desc layout, and the float64 restatement tests/microfacet64.py proven against itself before it judges the HIP kernels."""
import ctypes
import os
import subprocess
import tempfile
import numpy as np
import pytest
from mitsubaer_amd import host, params as P, capi
from tests import microfacet64 as mf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CAM = '<sensor type="perspective"><film type="hdrfilm"><integer name="width" value="8"/><integer name="height" value="8"/></film></sensor>'
MED = ('<medium type="homogeneous" id="m"><spectrum name="sigmaS" value="1"/><spectrum name="sigmaA" value="0.1"/></medium>')
POINT = '<emitter type="point"><point name="position" x="%g" y="%g" z="%g"/><spectrum name="intensity" value="5"/></emitter>'


def _scene(tmp_path, bsdf, extra="", shape="cube"):
    f = str(tmp_path / "s.xml")
    body = ('<integrator type="volpath"/>' + CAM + MED + '<shape type="%s">%s<ref name="interior" id="m"/></shape>' % (shape, bsdf) + extra)
    open(f, "w").write('<scene version="0.5.0">' + body + '</scene>')
    return f


def test_xml_flattening_and_defaults(tmp_path):
    d, _ = host.flatten_xml(_scene(tmp_path, '<bsdf type="hroughdielectric"/>'))
    assert d.boundary_bsdf == P.BSDF_HROUGHDIELECTRIC == 2
    assert d.rough_distribution == P.MICROFACET_BECKMANN and abs(d.rough_alpha - 0.1) < 1e-7 and d.rough_sample_visible == 1
    for name, kind in (("beckmann", P.MICROFACET_BECKMANN), ("ggx", P.MICROFACET_GGX), ("GGX", P.MICROFACET_GGX)):
        b = '<bsdf type="hroughdielectric"><string name="distribution" value="%s"/><float name="alpha" value="0.3"/>' \
            '<boolean name="sampleVisible" value="false"/></bsdf>' % name
        d, _ = host.flatten_xml(_scene(tmp_path, b))
        assert d.rough_distribution == kind and abs(d.rough_alpha - 0.3) < 1e-7 and d.rough_sample_visible == 0
    # phong: visible sampling forced off (microfacet.h:137-142)
    b = '<bsdf type="hroughdielectric"><string name="distribution" value="phong"/><boolean name="sampleVisible" value="true"/></bsdf>'
    d, _ = host.flatten_xml(_scene(tmp_path, b))
    assert d.rough_distribution == P.MICROFACET_PHONG and d.rough_sample_visible == 0
    # alpha clamp (microfacet.h:131-136) and equal alphaU / alphaV
    d, _ = host.flatten_xml(_scene(tmp_path, '<bsdf type="hroughdielectric"><float name="alpha" value="0"/></bsdf>'))
    assert abs(d.rough_alpha - 1e-4) < 1e-10
    d, _ = host.flatten_xml(_scene(tmp_path, '<bsdf type="hroughdielectric"><float name="alphaU" value="0.2"/><float name="alphaV" value="0.2"/></bsdf>'))
    assert abs(d.rough_alpha - 0.2) < 1e-7
    # the other boundaries keep all-zero rough fields
    d, _ = host.flatten_xml(_scene(tmp_path, '<bsdf type="hdielectric"/>'))
    assert d.boundary_bsdf == P.BSDF_HDIELECTRIC and (d.rough_distribution, d.rough_alpha, d.rough_sample_visible) == (0, 0.0, 0)
    # an outside point emitter is accepted
    d, _ = host.flatten_xml(_scene(tmp_path, '<bsdf type="hroughdielectric"/>', POINT % (0, 3, 0)))
    assert list(d.point_position) == [0, 3, 0]


AREA = ('<shape type="rectangle"><transform name="toWorld"><translate x="0" y="3" z="0"/></transform>'
        '<emitter type="area"><spectrum name="radiance" value="1"/></emitter></shape>')


@pytest.mark.parametrize("bsdf,extra,shape,msg", [
    ('<bsdf type="hroughdielectric"/>', POINT % (0.2, 0.1, 0), "cube", "point emitter must lie outside"),
    ('<bsdf type="hroughdielectric"/>', POINT % (0.2, 0.1, 0), "sphere", "point emitter must lie outside"),
    ('<bsdf type="hroughdielectric"/>', AREA, "cube", "area emitter"),
    ('<bsdf type="hroughdielectric"><string name="distribution" value="as"/></bsdf>', "", "cube", "anisotropic 'as'"),
    ('<bsdf type="hroughdielectric"><string name="distribution" value="foo"/></bsdf>', "", "cube", "invalid distribution"),
    ('<bsdf type="hroughdielectric"><float name="alphaU" value="0.1"/><float name="alphaV" value="0.2"/></bsdf>', "", "cube", "anisotropic roughness"),
    ('<bsdf type="hroughdielectric"><float name="alphaU" value="0.1"/></bsdf>', "", "cube", "alphaU'/'alphaV"),
    ('<bsdf type="hroughdielectric"><texture name="alpha" type="bitmap"/></bsdf>', "", "cube", "texture"),
    ('<bsdf type="hroughdielectric"><spectrum name="specularReflectance" value="0.5"/></bsdf>', "", "cube", "specularReflectance"),
    ('<bsdf type="hroughdielectric"><spectrum name="specularTransmittance" value="0.5"/></bsdf>', "", "cube", "specularTransmittance"),
])
def test_host_refusals(tmp_path, bsdf, extra, shape, msg):
    with pytest.raises(host.HostError, match=msg):
        host.flatten_xml(_scene(tmp_path, bsdf, extra, shape))


def _rough_params(**kw):
    p = P.SceneParams(width=8, height=8, sigma_mode=P.SIGMA_HOMOGENEOUS)
    p.boundary_bsdf = P.BSDF_HROUGHDIELECTRIC
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def _ball(N=24):
    from mitsubaer_amd import synth
    return -synth.sphere_sdf(N, radius=0.9, aabb_min=[-1.05] * 3, aabb_max=[1.05] * 3)


@pytest.mark.parametrize("kw,msg", [
    (dict(point_position=[0.1, 0.2, 0.0], point_intensity=[1, 1, 1]), "point emitter must lie outside"),
    (dict(boundary=P.BOUNDARY_SPHERE, point_position=[0.1, 0.2, 0.0], point_intensity=[1, 1, 1]), "point emitter must lie outside"),
    (dict(area_radiance=[1, 1, 1]), "area emitter"),
    (dict(rough_distribution=3), "distribution"),
    (dict(rough_alpha=-0.1), "alpha"),
    (dict(rough_alpha=float("nan")), "alpha"),
    (dict(boundary_bsdf=3), "boundary BSDF"),
    (dict(boundary=P.BOUNDARY_SDF, sdf=_ball(), sdf_aabb=([-1.05] * 3, [1.05] * 3), point_position=[0.1, 0.2, 0.0], point_intensity=[1, 1, 1]),
     "point emitter must lie outside"),
])
def test_capi_refusals(kw, msg):
    with pytest.raises(capi.MerError, match=msg):
        capi.validate_rough(_rough_params(**kw))
    capi.validate_rough(_rough_params(point_position=[0.0, 3.0, 0.0], point_intensity=[1, 1, 1]))     # outside: accepted
    capi.validate_rough(_rough_params(boundary=P.BOUNDARY_SDF, sdf=_ball(), sdf_aabb=([-1.05] * 3, [1.05] * 3), point_position=[0.0, 0.96, 0.0],
                                      point_intensity=[1, 1, 1]))           # inside the SDF's box, outside its shape: accepted


def test_scene_desc_layout_matches_the_header():
    src = ('#include "mer.h"\n#include <stdio.h>\n#include <stddef.h>\n'
           'int main(){printf("%zu %zu\\n", sizeof(mer_scene_desc), offsetof(mer_scene_desc, rough_distribution));return 0;}\n')
    with tempfile.TemporaryDirectory() as d:
        open(os.path.join(d, "t.c"), "w").write(src)
        subprocess.check_call(["gcc", "-I", os.path.join(ROOT, "include"), "-o", os.path.join(d, "t"), os.path.join(d, "t.c")])
        size, off = map(int, subprocess.check_output([os.path.join(d, "t")]).split())
    assert ctypes.sizeof(capi.SceneDesc) == size
    assert capi.SceneDesc.rough_distribution.offset == off and off == size - 12      # appended at the end


# ---- float64 self-checks of tests/microfacet64.py

def _dirs(n, seed, upper=None):
    v = np.random.RandomState(seed).normal(size=(n, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    if upper is not None:
        v[:, 2] = np.abs(v[:, 2]) * (1 if upper else -1)
    return v


KINDS = [(mf.BECKMANN, True), (mf.BECKMANN, False), (mf.GGX, True), (mf.GGX, False), (mf.PHONG, False)]


def test_frame_is_orthonormal_and_right_handed():
    for n in _dirs(50, 3):
        s, t = mf.frame(n)
        M = np.stack([s, t, n])
        assert np.allclose(M @ M.T, np.eye(3), atol=1e-12) and abs(np.linalg.det(M) - 1) < 1e-12


@pytest.mark.parametrize("kind,visible", KINDS)
@pytest.mark.parametrize("upper", [True, False])
def test_float64_sampler_chisquare_against_its_pdf(kind, visible, upper):
    d = mf.Distr(kind, 0.3, visible)
    rng = np.random.RandomState(11)
    n = 200000
    for wi in _dirs(3, 5 + upper, upper):
        wo, w, pdf, _ = mf.sample(d, 1.5, np.repeat(wi[None], n, 0), rng.rand(n, 3))
        pval, level = mf.chi2_sphere(wo, w > 0, n, mf.chi2_pdf(d, 1.5, wi))
        assert pval >= level, (pval, level, wi)


@pytest.mark.parametrize("kind,visible", KINDS)
def test_float64_sampler_weight_is_eval_over_pdf_and_mean_is_albedo(kind, visible):
    d = mf.Distr(kind, 0.3, visible)
    rng = np.random.RandomState(2)
    for wi in (np.array([0.3, -0.2, 0.93]), np.array([0.6, 0.1, -0.79])):
        wi = wi / np.linalg.norm(wi)
        n = 400000
        wo, w, pdf, _ = mf.sample(d, 1.5, np.repeat(wi[None], n, 0), rng.rand(n, 3))
        ok = w > 0
        val, p2 = mf.eval_pdf(d, 1.5, np.repeat(wi[None], ok.sum(), 0), wo[ok])
        assert np.allclose(p2, pdf[ok], rtol=1e-9)
        assert np.allclose(val / p2, w[ok], rtol=1e-9)
        a = mf.albedo(d, 1.5, wi)
        assert abs(w.mean() - a) < 4 * w.std() / np.sqrt(n) + 1e-3 * a, (w.mean(), a)


@pytest.mark.parametrize("eta", [1.33, 1.5, 2.4])
@pytest.mark.parametrize("kind", [mf.BECKMANN, mf.GGX, mf.PHONG])
def test_float64_smooth_limit_reflectance_at_normal_incidence(kind, eta):
    d = mf.Distr(kind, 1e-3, True)
    n = 100000
    wo, w, pdf, _ = mf.sample(d, eta, np.repeat(np.array([[0.0, 0.0, 1.0]]), n, 0), np.random.RandomState(4).rand(n, 3))
    R = np.sum(w * (wo[:, 2] > 0)) / n
    F0 = ((eta - 1) / (eta + 1)) ** 2
    assert abs(R - F0) < 4 * np.sqrt(F0 * (1 - F0) / n) + 1e-3 * F0, (R, F0)


@pytest.mark.parametrize("kind,visible", KINDS)
def test_float64_reflection_lobe_is_reciprocal(kind, visible):
    d = mf.Distr(kind, 0.25, visible)
    for upper in (True, False):
        wi = _dirs(2000, 8, upper); wo = _dirs(2000, 9, upper)
        f1, _ = mf.eval_pdf(d, 1.5, wi, wo)
        f2, _ = mf.eval_pdf(d, 1.5, wo, wi)
        assert np.allclose(f1 / np.abs(wo[:, 2]), f2 / np.abs(wi[:, 2]), rtol=1e-10, atol=1e-300)
