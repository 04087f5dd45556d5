// mer_microfacet.hpp -- the rough dielectric boundary of the medium shape (MER_BSDF_HROUGHDIELECTRIC; the reference's
// src/bsdfs/hroughdielectric.cpp: eta is the RIF at the hit point, exterior index 1).  Written from the published models:
//   Walter, Marschner, Li, Torrance 2007, "Microfacet models for refraction through rough surfaces": the Beckmann, GGX and Phong
//   distributions, Smith masking (Beckmann's rational approximation, also used for Phong), the reflection / refraction BSDF, the
//   half-vector Jacobians, the alpha -> Phong exponent map 2 / alpha^2 - 2 and the sampling-alpha widening 1.2 - 0.2 sqrt|cos theta_i|;
//   Heitz, d'Eon 2014, "Importance sampling microfacet-based BSDFs using the distribution of visible normals": sampling of the visible
//   normals by stretching to alpha = 1, sampling the slopes (GGX x: the paper's closed form; GGX y and Beckmann x: the inverse of the exact
//   slope CDF, solved by safeguarded Newton steps) and unstretching.
// Conventions follow the reference (src/bsdfs/microfacet.h, hroughdielectric.cpp): isotropic alpha clamped to >= 1e-4, sampleVisible
// forced off for Phong, the lobe sampled around sign(cos theta_i) wi, ERadiance scaling (1/eta)^2 of refractions entering the medium.
// Vectors are in the local frame of the hit: z = the outward normal of the medium shape, wi and wo point away from the surface; eta =
// interior / exterior index.
#pragma once
#include "mer_device.hpp"

namespace mer {

struct Microfacet { int type; float alpha, exponent; int visible; };

__device__ __forceinline__ Microfacet microfacet_scaled(Microfacet d, float s) {            // MicrofacetDistribution::scaleAlpha
    d.alpha *= s;
    d.exponent = fmaxf(2.0f / (d.alpha * d.alpha) - 2.0f, 0.0f);
    return d;
}
__device__ __forceinline__ Microfacet microfacet_make(int type, float alpha, int sample_visible) {
    Microfacet d; d.type = type; d.alpha = 1.0f; d.visible = (sample_visible != 0 && type != MER_MICROFACET_PHONG) ? 1 : 0;
    return microfacet_scaled(d, fmaxf(alpha, 1e-4f));
}

// D(m): the microfacet normal density, normalised so that the integral of D(m) cos theta_m over the hemisphere is 1
__device__ __forceinline__ float mf_D(const Microfacet &d, f3 m) {
    if (m.z <= 0) return 0.0f;
    const float c2 = m.z * m.z, a2 = d.alpha * d.alpha, t2a = (m.x * m.x + m.y * m.y) / (c2 * a2);    // tan^2 theta / alpha^2
    if (d.type == MER_MICROFACET_GGX) { const float r = (1.0f + t2a) * c2; return 1.0f / (MER_PI * a2 * r * r); }
    if (d.type == MER_MICROFACET_PHONG) return (d.exponent + 2.0f) * (0.5f * MER_INV_PI) * powf(m.z, d.exponent);
    return expf(-t2a) / (MER_PI * a2 * c2 * c2);
}
// Smith's G1(v, m); zero when v sees the back of m
__device__ __forceinline__ float mf_G1(const Microfacet &d, f3 v, f3 m) {
    if (dot(v, m) * v.z <= 0) return 0.0f;
    const float tanTheta = fabsf(sqrtf(fmaxf(0.0f, 1.0f - v.z * v.z)) / v.z);
    if (tanTheta == 0.0f) return 1.0f;
    if (d.type == MER_MICROFACET_GGX) { const float r = d.alpha * tanTheta; return 2.0f / (1.0f + sqrtf(1.0f + r * r)); }
    const float a = 1.0f / (d.alpha * tanTheta);
    if (a >= 1.6f) return 1.0f;
    return (3.535f * a + 2.181f * a * a) / (1.0f + 2.276f * a + 2.577f * a * a);
}
// density of the visible normals seen from v (v.z > 0), or of D(m) cos theta_m for the full sampler
__device__ __forceinline__ float mf_pdf(const Microfacet &d, f3 v, f3 m) {
    if (!d.visible) return mf_D(d, m) * m.z;
    if (v.z == 0) return 0.0f;
    return mf_D(d, m) * mf_G1(d, v, m) * fabsf(dot(v, m)) / v.z;
}

// slopes of the alpha = 1 distribution's visible normals seen at inclination theta (cos theta = ci), azimuth 0
__device__ __forceinline__ void mf_sample11(int type, float ci, float u1, float u2, float &sx, float &sy) {
    const float si = sqrtf(fmaxf(0.0f, 1.0f - ci * ci));
    if (type == MER_MICROFACET_GGX) {
        if (ci > 0.9999f) {                                       // normal incidence: the slope distribution itself
            const float r = sqrtf(u1 / (1.0f - u1)), phi = 2.0f * MER_PI * u2;
            sx = r * cosf(phi); sy = r * sinf(phi); return;
        }
        const float tanI = si / ci, G1 = 2.0f / (1.0f + sqrtf(1.0f + tanI * tanI));
        const float A = 2.0f * u1 / G1 - 1.0f;                   // in [-1, 1 / cos theta)
        const float den = A * A - 1.0f;
        const float tmp = 1.0f / (fabsf(den) < 1e-10f ? copysignf(1e-10f, den) : den), B = tanI;
        const float D = sqrtf(fmaxf(B * B * tmp * tmp - (A * A - B * B) * tmp, 0.0f));
        const float x1 = B * tmp - D, x2 = B * tmp + D;
        sx = (A < 0 || x2 > 1.0f / tanI) ? x1 : x2;
        // y given x: sqrt(1 + x^2) tan(phi), phi with density cos^2(phi) / (pi / 2) on (-pi/2, pi/2), i.e. the root of
        // phi + sin(phi) cos(phi) = pi (u2 - 1/2): safeguarded Newton steps (the inverse of the exact conditional CDF)
        const float t = MER_PI * (u2 - 0.5f);
        float lo = -0.5f * MER_PI, hi = 0.5f * MER_PI, ph = 0.5f * t;
        for (int it = 0; it < 24; ++it) {
            const float sp = sinf(ph), cp = cosf(ph), f = ph + sp * cp - t;
            if (f > 0) hi = ph; else lo = ph;
            const float pn = ph - f / (2.0f * cp * cp);
            const float next = (pn > lo && pn < hi) ? pn : 0.5f * (lo + hi);
            if (fabsf(next - ph) <= 1e-7f) { ph = next; break; }
            ph = next;
        }
        sy = tanf(ph) * sqrtf(1.0f + sx * sx);
        return;
    }
    // Beckmann: the x slope has density (ci - x si) exp(-x^2) on x < cot theta; its CDF (up to a constant) is
    // C(x) = ci sqrt(pi)/2 erfc(-x) + si/2 exp(-x^2).  The y slope is an independent unit Gaussian / sqrt(2).
    const float hi0 = si > 0 ? fminf(ci / si, 8.0f) : 8.0f;
    const float k = 0.5f * sqrtf(MER_PI) * ci;
    const float target = u1 * (k * erfcf(-hi0) + 0.5f * si * expf(-hi0 * hi0));
    float lo = -8.0f, hi = hi0, x = fminf(0.0f, hi0);
    for (int it = 0; it < 32; ++it) {
        const float e = expf(-x * x), f = k * erfcf(-x) + 0.5f * si * e - target;
        if (f > 0) hi = x; else lo = x;
        const float p = (ci - x * si) * e, xn = x - f / p;
        const float next = (xn > lo && xn < hi) ? xn : 0.5f * (lo + hi);
        if (fabsf(next - x) <= 1e-6f * fmaxf(1.0f, fabsf(x))) { x = next; break; }
        x = next;
    }
    sx = x;
    sy = erfinvf(fminf(fmaxf(2.0f * u2 - 1.0f, -0.99999988f), 0.99999988f));
}
// a visible normal seen from v (v.z > 0): stretch, sample the alpha = 1 slopes, rotate, unstretch
__device__ __forceinline__ f3 mf_sample_visible(const Microfacet &d, f3 v, float u1, float u2) {
    const f3 vs = normalize(f3(d.alpha * v.x, d.alpha * v.y, v.z));
    const float st = sqrtf(fmaxf(0.0f, 1.0f - vs.z * vs.z));
    const float cp = st > 0 ? vs.x / st : 1.0f, sp = st > 0 ? vs.y / st : 0.0f;
    float sx, sy;
    mf_sample11(d.type, vs.z, u1, u2, sx, sy);
    const float rx = (cp * sx - sp * sy) * d.alpha, ry = (sp * sx + cp * sy) * d.alpha;
    return normalize(f3(-rx, -ry, 1.0f));
}
// a normal from D(m) cos theta_m; pdf = D(m) cos theta_m
__device__ __forceinline__ f3 mf_sample_all(const Microfacet &d, float u1, float u2, float &pdf) {
    float cosT;
    if (d.type == MER_MICROFACET_PHONG) cosT = powf(u1, 1.0f / (d.exponent + 2.0f));
    else {
        const float a2 = d.alpha * d.alpha;
        const float t2 = d.type == MER_MICROFACET_GGX ? a2 * u1 / (1.0f - u1) : -a2 * logf(1.0f - u1);
        cosT = 1.0f / sqrtf(1.0f + t2);
    }
    const float sinT = sqrtf(fmaxf(0.0f, 1.0f - cosT * cosT)), phi = 2.0f * MER_PI * u2;
    const f3 m(sinT * cosf(phi), sinT * sinf(phi), cosT);
    pdf = mf_D(d, m) * cosT;
    return m;
}

// the sampling distribution of the reference: the visible normals, or the full distribution with Walter's widened alpha
__device__ __forceinline__ Microfacet rough_sampling_distr(const Microfacet &d, float cosI) {
    return d.visible ? d : microfacet_scaled(d, 1.2f - 0.2f * sqrtf(fabsf(cosI)));
}

// f |cos theta_o| (ERadiance) and the solid-angle pdf of sampling wo
__device__ __forceinline__ float rough_dielectric_eval(const Microfacet &d, float eta, f3 wi, f3 wo, float &pdf) {
    pdf = 0.0f;
    const float ci = wi.z, co = wo.z;
    if (ci == 0) return 0.0f;
    const bool refl = ci * co > 0;
    const float etaR = refl ? 1.0f : (ci > 0 ? eta : 1.0f / eta);
    f3 H = refl ? normalize(wo + wi) : normalize(wi + wo * etaR);
    if (H.z < 0) H = -H;
    const float D = mf_D(d, H);
    if (D == 0) return 0.0f;
    float cosT; const float F = fresnel_dielectric_ext(dot(wi, H), cosT, eta);
    const float G = mf_G1(d, wi, H) * mf_G1(d, wo, H);
    const float wiH = dot(wi, H), woH = dot(wo, H);
    const Microfacet sd = rough_sampling_distr(d, ci);
    const float prob = mf_pdf(sd, ci > 0 ? wi : -wi, H);
    float val, dwh_dwo;
    if (refl) {
        val = F * D * G / (4.0f * fabsf(ci));
        dwh_dwo = 1.0f / (4.0f * woH);
        pdf = fabsf(prob * F * dwh_dwo);
    } else {
        const float sqrtDenom = wiH + etaR * woH;
        const float factor = ci > 0 ? 1.0f / eta : eta;
        val = fabsf((1.0f - F) * D * G * etaR * etaR * wiH * woH / (ci * sqrtDenom * sqrtDenom)) * (factor * factor);
        dwh_dwo = etaR * etaR * woH / (sqrtDenom * sqrtDenom);
        pdf = fabsf(prob * (1.0f - F) * dwh_dwo);
    }
    return val;
}
// sample wo: u1, u2 = the microfacet normal, u3 = the reflect / refract choice.  Returns eval / pdf (0: no sample); etaS = the relative index
// of the sampled event (1 for a reflection; bRec.eta)
__device__ __forceinline__ float rough_dielectric_sample(const Microfacet &d, float eta, f3 wi, float u1, float u2, float u3, f3 &wo, float &pdf,
                                                         float &etaS) {
    pdf = 0.0f; etaS = 1.0f; wo = f3(0, 0, 1);
    const float ci = wi.z;
    if (ci == 0) return 0.0f;
    const Microfacet sd = rough_sampling_distr(d, ci);
    const f3 ws = ci > 0 ? wi : -wi;
    f3 m; float mpdf;
    if (sd.visible) { m = mf_sample_visible(sd, ws, u1, u2); mpdf = mf_pdf(sd, ws, m); }
    else m = mf_sample_all(sd, u1, u2, mpdf);
    if (!(mpdf > 0)) return 0.0f;
    const float wiM = dot(wi, m);
    float cosT; const float F = fresnel_dielectric_ext(wiM, cosT, eta);
    float weight = 1.0f, dwh_dwo;
    if (u3 <= F) {                                                    // reflection (chosen with probability F)
        pdf = mpdf * F;
        wo = m * (2.0f * wiM) - wi;
        if (ci * wo.z <= 0) return 0.0f;
        dwh_dwo = 1.0f / (4.0f * dot(wo, m));
    } else {
        pdf = mpdf * (1.0f - F);
        if (cosT == 0) return 0.0f;
        const float e = cosT < 0 ? 1.0f / eta : eta;                  // refract(wi, m, eta, cosThetaT)
        wo = m * (wiM * e + cosT) - wi * e;
        etaS = cosT < 0 ? eta : 1.0f / eta;
        if (ci * wo.z >= 0) return 0.0f;
        const float factor = cosT < 0 ? 1.0f / eta : eta;             // ERadiance: solid-angle compression
        weight = factor * factor;
        const float sqrtDenom = wiM + etaS * dot(wo, m);
        dwh_dwo = etaS * etaS * dot(wo, m) / (sqrtDenom * sqrtDenom);
    }
    if (sd.visible) weight *= mf_G1(d, wo, m);
    else weight *= fabsf(mf_D(d, m) * mf_G1(d, wi, m) * mf_G1(d, wo, m) * wiM / (mpdf * ci));
    pdf *= fabsf(dwh_dwo);
    return weight;
}

}  // namespace mer

namespace mer {

// HRoughDielectric at the boundary point ro + rd*t of the medium shape, as volpath's surface vertex (volpath.cpp:230-275).  Sampler draws,
// in this order: (1) the emitter sample, nextSample2D -- drawn whether or not the scene has a point emitter (the environment is not
// emitter-sampled); (2) the microfacet normal, nextSample2D; (3) the reflect / refract choice, next1D (hroughdielectric.cpp:430-437).
// Le = T x I / r^2 x eval(wi, wo_e) of a point emitter on the exterior side of the surface (delta emitter: MIS weight 1; the caller checks
// that it lies outside the shape) and eLen its distance (a vacuum edge).  On return T, etaPath carry the sampled event (ERadiance weight,
// bRec.eta).  Returns 0: no sample, the path ends; 1: wo leaves the shape; 2: wo stays in / enters the medium.
template <bool CURVED, int RIF, int BND = 0>
__device__ __forceinline__ int rough_event(const Params &P, Rng &rng, f3 ro, f3 rd, float t, f3 &T, float &etaPath, f3 &x, f3 &wo, f3 &Le,
                                           float &eLen) {
    const mer_scene_desc &S = P.sc;
    x = ro + rd * t;
    const f3 n = shape_normal_b<BND>(P, x);
    const float etaB = boundary_eta<CURVED, RIF>(P, x);
    f3 s, u;
    coordinate_system(n, s, u);                                   // Frame(n) (frame.h:55-57)
    const f3 wiW = -rd, wi(dot(wiW, s), dot(wiW, u), dot(wiW, n));
    const Microfacet d = microfacet_make(S.rough_distribution, S.rough_alpha, S.rough_sample_visible);
    (void) rng.next1D(); (void) rng.next1D();                     // (1)
    Le = f3(0, 0, 0); eLen = 0.0f;
    if (P.n_point) {
        float pk; const int k = emitter_select(P.points, P.n_point, rng, 3, pk);
        const DPoint &E = P.points[k];                            // one of the point emitters; E.Ie = I / its pdf
        f3 dv(E.pos[0] - x.x, E.pos[1] - x.y, E.pos[2] - x.z);
        const float dist = sqrtf(dot(dv, dv));
        dv = dv / dist;
        const f3 wl(dot(dv, s), dot(dv, u), dot(dv, n));
        // the exterior side of the surface: cube and sphere are convex, a signed-distance shape is sphere-traced along the segment, from just
        // off the surface
        bool visible = wl.z > 0;
        if (BND != 0 && visible) visible = intersect_shape_b<BND>(P, x + n * (8.0f * P.sdf_eps), dv, 0.0f, dist) < 0;
        if (visible) {
            float pdfE;
            const float f = rough_dielectric_eval(d, etaB, wi, wl, pdfE);
            const f3 I(E.Ie[0], E.Ie[1], E.Ie[2]);
            Le = T * I * (f / (dist * dist)) * point_falloff(spot_table(P), k, dv);     // a spot's cone (1 for a point emitter)
            eLen = dist;
        }
    }
    const float u1 = rng.next1D(), u2 = rng.next1D();             // (2)
    const float u3 = rng.next1D();                                // (3)
    f3 wl; float pdf, etaS;
    const float w = rough_dielectric_sample(d, etaB, wi, u1, u2, u3, wl, pdf, etaS);
    if (!(w > 0)) { T = f3(0, 0, 0); return 0; }
    wo = s * wl.x + u * wl.y + n * wl.z;                          // Frame::toWorld
    T = T * w;
    etaPath *= etaS;
    return wl.z > 0 ? 1 : 2;
}

}  // namespace mer
