// mer_ptracer.hpp -- light tracing (integrator = MER_INTEGRATOR_PTRACER): the reference's `ptracer` integrator and the t = 1 strategy of
// its `bdpt`.  ParticleTracer::process (src/librender/particleproc.cpp:107-270) with CaptureParticleWorker::handleMediumInteraction
// (src/integrators/ptracer/ptracer_proc.cpp:167-194) as the handler, restricted to one convex index-matched shape with an interior medium:
// a path starts at an emitter, enters the shape, and every scattering vertex is connected to the pinhole and splatted onto the pixel the
// connection arrives at.  It is the estimator for sources no camera path can sample (a collimated beam).
//
// One lane runs one light path to completion: a first, divergent megakernel built from the device functions the wavefront kernels use --
// Walk (free flights), phase_sample / phase_eval, Connector (curved connections), straight_transmittance, film_contribute / film_splat.
// Every loop has a bound: the path's step budget (PT_STEP_BUDGET march units), the solver's own caps (Connector: 20 iterations x 6 trials,
// 64 restarts, maxSteps per ray), the tracking loops of a connection (PT_TRACK_BUDGET) and PT_MAX_EVENTS scatterings; the host launches
// PT_PATHS_PER_LAUNCH (curved rays: PT_PATHS_PER_LAUNCH_CURVED) paths at a time.  Scheduling light paths in wavefronts is left to a later change.
#pragma once
#include "mer_walk.hpp"
#include "mer_connect.hpp"

namespace mer {

#define PT_BLOCK 64
#define PT_PATHS_PER_LAUNCH (1u << 20)       // paths per kernel launch, straight rays (mer_render_ptracer.hip): no launch runs long (measured: 7 ms)
#define PT_PATHS_PER_LAUNCH_CURVED (1u << 16)   // ... curved rays: one resident wave per SIMD of the chip (measured: 0.7 s with the acoustic example scene)
#define PT_MAX_EVENTS 4096                   // scatterings + boundary crossings of one path (Russian roulette ends paths long before)
#define PT_STEP_BUDGET (1u << 22)            // march units (eikonal steps / tentative collisions) of one path over all its free flights
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

// ---------------------------------------------------------------------------------------------------
// Emitter::sampleRay of point-table slot k: PointEmitter (src/emitters/point.cpp: uniform sphere, weight I 4 pi), SpotEmitter
// (spot.cpp:169-182: uniform cone of the cutoff angle about the axis, weight I falloffCurve / pdf) or CollimatedBeamEmitter
// (collimated.cpp:115-124: the fixed ray, weight = power).  E.Ie = intensity (power) / selection probability.  Two sampler numbers for a
// point or spot, none for a beam.  The cone is sampled in an orthonormal frame about the axis: the falloff depends on the polar angle only.
__device__ __forceinline__ f3 emit_ray(const Params &P, int k, Rng &rng, f3 &o, f3 &d) {
    const DPoint &E = P.points[k];
    o = f3(E.pos[0], E.pos[1], E.pos[2]);
    const f3 I(E.Ie[0], E.Ie[1], E.Ie[2]);
    const DSpot *spots = spot_table(P);
    if (spots && spots[k].pad != 0.0f) { d = f3(spots[k].z[0], spots[k].z[1], spots[k].z[2]); return I; }
    const float u1 = rng.next1D(), u2 = rng.next1D();
    if (spots && spots[k].cos_cutoff > -1.5f) {
        const DSpot &s = spots[k];
        const float cosTheta = (1.0f - u1) + u1 * s.cos_cutoff, sinTheta = safe_sqrt(1.0f - cosTheta * cosTheta), phi = u2 * (2.0f * MER_PI);   // warp.cpp:54-63
        const f3 a = normalize(f3(s.z[0], s.z[1], s.z[2])); f3 b, c;
        coordinate_system(a, b, c);
        d = b * (cosf(phi) * sinTheta) + c * (sinf(phi) * sinTheta) + a * cosTheta;
        const float invPdf = (2.0f * MER_PI) * (1.0f - s.cos_cutoff);
        return I * (spot_falloff(s, -d) * invPdf);
    }
    d = square_to_uniform_sphere(u1, u2);
    return I * (4.0f * MER_PI);
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
// K_ptracer: light path j = work id `first + j` of the shard = the (pixel, sample index) pair K_gen would enumerate (decode_work); its
// sampler stream is keyed by that pair.
template <bool CURVED, int RIF, int STEPPER, int SIGMA>
__global__ void __launch_bounds__(PT_BLOCK) ptracer_kernel(const Params P, uint64_t first, uint32_t count) {
    const mer_scene_desc &S = P.sc;
    const uint32_t j = blockIdx.x * PT_BLOCK + threadIdx.x;
    LaneCounters C; C.clear();
    int x = 0, y = 0; uint32_t sample = 0;
    bool live = j < count && decode_work(P, first + j, x, y, sample);        // a work id of a partial tile may fall outside the image
    if (live) {
        // the pair's unit of weight: exactly 1 into the pixel's alpha and weight (RGB / weight = accum x W H / particles)
        float *dest = P.film + MER_CHK(P.chk, CHK_FILM, ((size_t) y * S.width + x) * P.film_ch, P.n_film - (uint32_t) P.film_ch + 1u);
        atomicAdd(dest + P.film_ch - 2, 1.0f); atomicAdd(dest + P.film_ch - 1, 1.0f);
        C.paths++;
        Rng rng; rng.seed(P.seed, (uint32_t) (y * S.width + x), sample);
        const int maxDepth = S.max_depth;
        const f3 camO(S.cam_to_world[3], S.cam_to_world[7], S.cam_to_world[11]);
        const bool camInside = inside_shape(S, camO);

        // ---- emission (Scene::sampleEmitterRay: one emitter by samplingWeight, from a forked stream as emitter_select has it)
        float pk; const int k = emitter_select(P.points, P.n_point, rng, 3, pk);
        f3 ps, dcur;
        const f3 power = emit_ray(P, k, rng, ps, dcur);
        f3 T(1, 1, 1);
        float plen = 0.0f;
        int depth = 1;
        bool alive = !is_zero(power);
        bool entering = false;                                   // the next segment starts on the boundary (ray.mint = Epsilon)
        bool enteredShape = false;                               // the emitter lies outside: the path has crossed the null boundary (and paid one depth)
        // Russian roulette at the end of every loop trip of process() (:258-267): q = min(max throughput, 0.95), no eta^2
        auto roulette = [&]() {
            if (depth++ >= S.rr_depth) {
                const float q = fminf(max3(T), 0.95f);
                if (rng.next1D() >= q) alive = false; else T = T / q;
            }
        };
        if (alive && !inside_shape(S, ps)) {
            // an emitter outside the shape: the ray meets the null boundary (a surface vertex: one depth, as in volpath) or nothing
            if (depth <= maxDepth || maxDepth < 0) {
                const float tIn = intersect_shape(S, ps, dcur, 0.0f, MER_INF);
                if (tIn >= 0) {
                    plen += edge_length(P, tIn);                 // exterior index 1
                    ps = ps + dcur * tIn; entering = true; enteredShape = true;
                    roulette();
                } else alive = false;
            } else alive = false;
        }

        Walk<CURVED, RIF, STEPPER, SIGMA> W;
        for (int event = 0; alive && event < PT_MAX_EVENTS; ++event) {
            if (is_zero(T) || !(depth <= maxDepth || maxDepth < 0)) break;
            // ---- free flight (Medium::sampleDistance over [0, its.t]; curved: to the collision or the boundary)
            float itsT = 0.0f;
            if (!CURVED) { itsT = intersect_shape(S, ps, dcur, entering ? MER_EPSILON : 0.0f, MER_INF); if (!(itsT >= 0)) break; }
            entering = false;
            C.segments++;
            W.t = 0; W.tmin = 0; W.tmax = 0; W.n0 = 1; W.rem = 0; W.steps_left = 0; W.seg_inf = 0; W.sdens = 0; W.backstep = 0; W.hprev = 0; W.cc.reset();
            int ev = W.begin(P, rng, C, K_FREE, ps, dcur, itsT);
            float sigma = 0.0f;
            for (;;) {
                if (ev == EV_NONE) { if (C.marched >= PT_STEP_BUDGET) { ev = EV_GATE_FAIL; break; } ev = W.advance(P, rng, C); }
                else if (ev == EV_ARRIVED) ev = W.on_arrived(P, rng, C, sigma);
                else if (ev == EV_EXITED) ev = EV_FAIL;
                else break;
            }
            if (ev != EV_REAL) break;           // the path left the convex shape (no further surface: process() :187-189) or its budget ran out
            MRec m;
            finish_free_flight(P, C, W, true, sigma, m);
            if (SIGMA == MER_SIGMA_HOMOGENEOUS && m.p.x == ps.x && m.p.y == ps.y && m.p.z == ps.z) break;       // no forward progress
            C.real++;
            plen += edge_length(P, CURVED ? m.opticalLength : m.t * S.rif_const);
            T = T * (m.sigmaS * m.transmittance / m.pdfSuccess);                                                 // :174
            const f3 wi = CURVED ? normalize(-m.d) : -W.v;
            ps = m.p;

            // ---- handleMediumInteraction (ptracer_proc.cpp:167-194): connect the vertex to the sensor
            if (!is_zero(T) && !(depth >= maxDepth && maxDepth > 0)) {
                const int interactions = maxDepth - depth - 1;   // null-boundary crossings the connection may make (scene.cpp sampleAttenuatedSensorDirect)
                float u, v, dist; f3 dS;
                const float imp = sensor_direct(P, ps, u, v, dS, dist);
                // Straight rays: the crossing is counted, as Scene::evalTransmittance and volpath's straight kernels count it.  Curved rays: volpath
                // charges a path ONE null crossing at most -- the camera's; K_connect does not count the crossing of its connection to an emitter
                // outside the shape -- and so does the light tracer: a path that has paid for entering the shape is not charged again.  Light
                // tracing and path tracing then hold the same scattering orders at every max_depth, with either kind of ray.
                const bool blocked = !camInside && interactions == 0 && !(CURVED && enteredShape);
                if (imp > 0 && !blocked) {
                    C.nee++;
                    if (!CURVED) {
                        const float tExit = intersect_shape(S, ps, dS, 0.0f, MER_INF);
                        const bool crosses = tExit >= 0 && tExit < dist;
                        const float L = crosses ? tExit : dist;
                        const f3 tr = straight_transmittance<SIGMA>(P, rng, C, ps, dS, L);
                        const f3 value = T * power * tr * (imp * phase_eval(S.phase, S.g, wi, dS));
                        float pl = plen + edge_length(P, L * S.rif_const);
                        if (crosses && camera_edge_counts(P)) pl += edge_length(P, dist - L);
                        light_splat(P, u, v, value, pl);
                    } else {
                        Connector<RIF, 0, true> K(P);
                        float w = 1.0f, optDist = 0, distIn = 0; f3 dir(0, 0, 0), rev(0, 0, 0);
                        if (K.connect(ps, camO, rng, w, dir, rev, optDist, distIn) && sensor_position(P, rev, u, v)) {   // the pixel of the ARRIVAL direction
                            const f3 tr = curved_transmittance<RIF, STEPPER, SIGMA>(P, rng, C, ps, dir, distIn);
                            const f3 value = T * power * tr * (imp * w * phase_eval(S.phase, S.g, wi, normalize(dir)));
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
            }
            // ---- phase-function sampling (EImportance; hg and isotropic are symmetric), then the roulette
            const float p2x = rng.next1D(), p2y = rng.next1D();
            f3 wo; float phasePdf;
            const float pw = phase_sample(S.phase, S.g, wi, p2x, p2y, wo, phasePdf);
            T = T * pw;
            dcur = wo;
            roulette();
        }
    }
    // counters: one wave-aggregated flush (every lane of the wave gets here)
    const uint32_t sums[8] = {wave_sum(C.paths), wave_sum(C.steps), wave_sum(C.rif_evals), wave_sum(C.tentative), wave_sum(C.real), wave_sum(C.segments),
                              wave_sum(C.nee), wave_sum(C.marched)};
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *dst = P.counters + (size_t) (blockIdx.x % MER_COUNTER_REPLICAS) * MER_C_COUNT;
#pragma unroll
        for (int q = 0; q < 7; q++) if (sums[q]) atomicAdd(dst + q, (unsigned long long) sums[q]);
        if (sums[7]) atomicAdd(dst + MER_C_ACTIVE_LANES, (unsigned long long) sums[7]);
    }
}

}  // namespace mer
