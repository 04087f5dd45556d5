// mer_ptracer.hpp -- light tracing (integrator = MER_INTEGRATOR_PTRACER): the reference's `ptracer` integrator and the t = 1 strategy of
// its `bdpt`.  ParticleTracer::process (src/librender/particleproc.cpp:107-270) with CaptureParticleWorker::handleMediumInteraction
// (src/integrators/ptracer/ptracer_proc.cpp:167-194) as the handler, restricted to one convex index-matched shape with an interior medium:
// a path starts at an emitter, enters the shape, and every scattering vertex is connected to the pinhole and splatted onto the pixel the
// connection arrives at.  It is the estimator for sources no camera path can sample (a collimated beam).
//
// One lane runs one light path to completion (LightPath, mer_lightpath.hpp): a first, divergent megakernel built from the device functions
// the wavefront kernels use -- Walk (free flights), phase_sample / phase_eval, Connector (curved connections), straight_transmittance,
// film_contribute / film_splat.  Beyond the bounds of the walk, the solver has its own caps (Connector: 20 iterations x 6 trials, 64
// restarts, maxSteps per ray) and the tracking loops of a connection have PT_TRACK_BUDGET.  Scheduling light paths in wavefronts is left to
// a later change.
#pragma once
#include "mer_lightpath.hpp"
#include "mer_connect.hpp"

namespace mer {

#define PT_TRACK_BUDGET (1u << 16)           // tentative collisions of one connection's transmittance estimate

// ---------------------------------------------------------------------------------------------------
// The pinhole as the end of a light path.  cam_to_world is rigid (make_params refuses anything else for the light tracer): the inverse
// of its linear part is the transpose.  cameraToSample at depth z, from sample_ray's inverse at the near plane:
//   sx = (1 - cot x / z) / 2,  sy = (1 - aspect cot y / z) / 2;  m_imageRect at z = 1: |x| <= 1 / cot, |y| <= 1 / (aspect cot).
__device__ __forceinline__ f3 sensor_to_local(const Params &P, f3 w) {
    const float *c = P.sc.cam_to_world;
    return f3(c[0] * w.x + c[4] * w.y + c[8] * w.z, c[1] * w.x + c[5] * w.y + c[9] * w.z, c[2] * w.x + c[6] * w.y + c[10] * w.z);
}
// PerspectiveCamera::importance (src/sensors/perspective.cpp:191-245) of the unit local direction d
__device__ __forceinline__ float sensor_importance(const Params &P, f3 d) {
    const float cosTheta = d.z;
    if (cosTheta <= 0) return 0.0f;
    const float invCosTheta = 1.0f / cosTheta;
    const float px = d.x * invCosTheta, py = d.y * invCosTheta;
    const float hx = 1.0f / P.cot_half_fov, hy = 1.0f / (P.aspect * P.cot_half_fov);
    if (!(px >= -hx && px <= hx && py >= -hy && py <= hy)) return 0.0f;
    const float normalization = 1.0f / ((2.0f * hx) * (2.0f * hy));                  // 1 / m_imageRect.getVolume()
    return normalization * invCosTheta * invCosTheta * invCosTheta;
}
// getSamplePosition (perspective.cpp:367-385) of a local direction / point: the film position in pixels; false behind the sensor or
// outside the frame
__device__ __forceinline__ bool sensor_local_to_film(const Params &P, f3 local, float &u, float &v) {
    u = v = 0.0f;
    if (!(local.z > 0)) return false;
    const float invz = 1.0f / local.z;
    const float sx = 0.5f - 0.5f * P.cot_half_fov * (local.x * invz), sy = 0.5f - 0.5f * (P.aspect * P.cot_half_fov) * (local.y * invz);
    if (!(sx >= 0 && sx <= 1 && sy >= 0 && sy <= 1)) return false;
    u = sx * (float) P.sc.width; v = sy * (float) P.sc.height;
    return true;
}
__device__ __forceinline__ bool sensor_position(const Params &P, f3 dir_world, float &u, float &v) {
    return sensor_local_to_film(P, sensor_to_local(P, dir_world), u, v);
}
// PerspectiveCamera::sampleDirect (perspective.cpp:387-424): importance x invDist^2 (0 outside the clip range or the frustum), the film
// position, the unit direction from ref to the sensor and the distance
__device__ __forceinline__ float sensor_direct(const Params &P, f3 ref, float &u, float &v, f3 &d, float &dist) {
    const float *c = P.sc.cam_to_world;
    const f3 o(c[3], c[7], c[11]);
    const f3 refP = sensor_to_local(P, ref - o);
    u = v = 0.0f; d = f3(0, 0, 0); dist = 0.0f;
    if (!(refP.z >= P.sc.near_clip && refP.z <= P.sc.far_clip)) return 0.0f;
    float uu, vv;
    if (!sensor_local_to_film(P, refP, uu, vv)) return 0.0f;
    const float len = sqrtf(dot(refP, refP)), invDist = 1.0f / len;
    const float imp = sensor_importance(P, refP * invDist);
    if (!(imp > 0)) return 0.0f;
    u = uu; v = vv; dist = len; d = (o - ref) * invDist;
    return imp * invDist * invDist;
}

// Medium::evalTransmittance along a found curved connection: arc length `dist` inside the shape, launched from ps with optical momentum dir
// (the estimator of connection_value, mer_connect.hpp: closed form for a homogeneous sigma_t, else ratio tracking or the two-walk Woodcock
// estimator along the re-traced ray)
template <int RIF, int STEPPER, int SIGMA>
__device__ __forceinline__ f3 curved_transmittance(const Params &P, Rng &rng, LaneCounters &C, f3 ps, f3 dir, float dist) {
    const mer_scene_desc &S = P.sc;
    if (SIGMA == MER_SIGMA_HOMOGENEOUS) return homogeneous_transmittance(P, -dist);
    const int nwalks = S.tr_estimator == MER_TR_WOODCOCK2 ? 2 : 1;
    float result = 0.0f; uint32_t budget = PT_TRACK_BUDGET;
    for (int wk = 0; wk < nwalks; ++wk) {
        f3 p = ps, v = dir; float left = dist, Tr = 1.0f, opt = 0; CellCache cc; cc.reset();
        while (budget) {
            budget--;
            const float s = -logf(1 - rng.next1D()) * P.inv_max_density;
            if (s >= left) break;
            const float h = S.stepsize; int steps = (int) (s / h); const float rem = s - steps * h; bool inside = true;
            for (int q = 0; q <= steps && inside; ++q) {
                const float hq = q < steps ? h : rem;
                er_step<RIF, STEPPER>(P.rif, cc, p, v, hq, opt); C.steps++;
                if (!inside_shape(S, p)) { er_step<RIF, STEPPER>(P.rif, cc, p, v, -hq, opt); C.steps++; inside = false; }
            }
            if (!inside) break;
            left -= s;
            const float sigma = lookup_float(P.density, p) * S.density_scale; C.tentative++;
            if (S.tr_estimator == MER_TR_RATIO) { Tr *= 1.0f - sigma * P.inv_max_density; if (Tr == 0.0f) break; }
            else if (sigma * P.inv_max_density > rng.next1D()) { Tr = 0.0f; break; }
        }
        result += Tr;
    }
    const float tv = result / (float) nwalks;
    return f3(tv, tv, tv);
}

// one contribution onto the film at (u, v): binned by path length (transient / bounce), weighted by the correlation function (modulated),
// or into the steady frame -- RGB only, with the filter's table weights (ImageBlock::put)
__device__ __forceinline__ void light_splat(const Params &P, float u, float v, f3 value, float pathLength) {
    if (is_zero(value)) return;
    if (P.sc.decomposition && !P.sc.modulation) film_contribute(P, u, v, value, pathLength);
    else film_splat(P, u, v, mod_weight<true>(P, value, pathLength), 0.0f, 0, 1);
}

// ---------------------------------------------------------------------------------------------------
// K_ptracer: the event loop is lane-divergent -- a lane leaves it when its path ends -- since nothing after it needs the wave together
// but the counter flush.
template <bool CURVED, int RIF, int STEPPER, int SIGMA>
__global__ void __launch_bounds__(PT_BLOCK) ptracer_kernel(const Params P, uint64_t first, uint32_t count) {
    const mer_scene_desc &S = P.sc;
    LaneCounters C; C.clear();
    LightPath<CURVED, SIGMA> lp;
    int x, y; float tIn;
    if (lp.decode(P, C, first, count, x, y)) {
        // the pair's unit of weight: exactly 1 into the pixel's alpha and weight (RGB / weight = accum x W H / particles)
        float *dest = P.film + MER_CHK(P.chk, CHK_FILM, ((size_t) y * S.width + x) * P.film_ch, P.n_film - (uint32_t) P.film_ch + 1u);
        atomicAdd(dest + P.film_ch - 2, 1.0f); atomicAdd(dest + P.film_ch - 1, 1.0f);
        const int maxDepth = lp.maxDepth;
        const f3 camO(S.cam_to_world[3], S.cam_to_world[7], S.cam_to_world[11]);
        const bool camInside = inside_shape(S, camO);
        const bool enteredShape = lp.emit(P, tIn) == LP_ENTERED;             // the emitter lies outside: the path has crossed the null boundary (and paid one depth)
        float plen = 0.0f;
        if (enteredShape) plen += edge_length(P, tIn);           // exterior index 1

        Walk<CURVED, RIF, STEPPER, SIGMA> W;
        for (int event = 0; lp.alive && event < PT_MAX_EVENTS; ++event) {
            if (!lp.can_fly()) break;
            const float itsT = lp.boundary_distance(S);
            if (!(itsT >= 0)) break;
            float sigma = 0.0f;
            const int ev = lp.run_flight(P, C, W, lp.begin_flight(P, C, W, itsT), sigma);
            if (ev != EV_REAL) break;           // the path left the convex shape or its budget ran out
            MRec m;
            if (!lp.collide(P, C, W, sigma, m)) break;
            plen += edge_length(P, CURVED ? m.opticalLength : m.t * S.rif_const);
            const f3 wi = lp.arrive(W, m);

            // ---- handleMediumInteraction (ptracer_proc.cpp:167-194): connect the vertex to the sensor
            if (!is_zero(lp.T) && !(lp.depth >= maxDepth && maxDepth > 0)) {
                Rng rng = lp.rng;                                // a copy: the solver is a call that takes the sampler's address, and lp stays in registers
                const int interactions = maxDepth - lp.depth - 1;   // null-boundary crossings the connection may make (scene.cpp sampleAttenuatedSensorDirect)
                float u, v, dist; f3 dS;
                const float imp = sensor_direct(P, lp.ps, u, v, dS, dist);
                // Straight rays: the crossing is counted, as Scene::evalTransmittance and volpath's straight kernels count it.  Curved rays: volpath
                // charges a path ONE null crossing at most -- the camera's; K_connect does not count the crossing of its connection to an emitter
                // outside the shape -- and so does the light tracer: a path that has paid for entering the shape is not charged again.  Light
                // tracing and path tracing then hold the same scattering orders at every max_depth, with either kind of ray.
                const bool blocked = !camInside && interactions == 0 && !(CURVED && enteredShape);
                if (imp > 0 && !blocked) {
                    C.nee++;
                    if (!CURVED) {
                        const float tExit = intersect_shape(S, lp.ps, dS, 0.0f, MER_INF);
                        const bool crosses = tExit >= 0 && tExit < dist;
                        const float L = crosses ? tExit : dist;
                        const f3 tr = straight_transmittance<SIGMA>(P, rng, C, lp.ps, dS, L);
                        const f3 value = lp.T * lp.power * tr * (imp * phase_eval(S.phase, S.g, wi, dS));
                        float pl = plen + edge_length(P, L * S.rif_const);
                        if (crosses && camera_edge_counts(P)) pl += edge_length(P, dist - L);
                        light_splat(P, u, v, value, pl);
                    } else {
                        Connector<RIF, 0, true> K(P);
                        float w = 1.0f, optDist = 0, distIn = 0; f3 dir(0, 0, 0), rev(0, 0, 0);
                        if (K.connect(lp.ps, camO, rng, w, dir, rev, optDist, distIn) && sensor_position(P, rev, u, v)) {   // the pixel of the ARRIVAL direction
                            const f3 tr = curved_transmittance<RIF, STEPPER, SIGMA>(P, rng, C, lp.ps, dir, distIn);
                            const f3 value = lp.T * lp.power * tr * (imp * w * phase_eval(S.phase, S.g, wi, normalize(dir)));
                            // the exterior leg is straight: from the sensor along rev back to the shape
                            float ext = 0.0f;
                            if (!camInside) { ext = intersect_shape(S, camO, rev, 0.0f, MER_INF); if (!(ext >= 0) || ext > optDist) ext = 0.0f; }
                            float pl = plen + edge_length(P, optDist - ext);
                            if (!camInside && camera_edge_counts(P)) pl += edge_length(P, ext);
                            light_splat(P, u, v, value, pl);
                        }
                        C.steps += K.nsteps;
                    }
                }
                lp.rng = rng;
            }
            lp.scatter(S, wi);
        }
    }
    flush_counters(P, C);
}

}  // namespace mer
