// mer_exitance.hpp -- where and when light paths leave the medium: a map of the escaped weight over the boundary of the medium shape
// (mer_render_exitance), a grid of the reference's `irradiancemeter` probes (src/sensors/irradiancemeter.cpp, driven by `ptracer`) instead of
// one probe per render.
//
// A light path is exactly the one K_fluence (mer_fluence.hpp) walks for the same scene, shard and seed -- work id and sampler key,
// emitter_select, emit_ray, the entry into the shape (one depth for the null boundary), the free flights, phase_sample, the roulette,
// PT_MAX_EVENTS and PT_STEP_BUDGET.  Recording an exit draws no sampler number, fetches no RIF value and advances no counter, so counters,
// paths, escaped weight and ended paths equal K_fluence's.  At each place where K_fluence sets `escaped = T * power` the lane notes the exit
// point x, the outward direction d, w = T power and the optical path length l (mer.h, mer_render_exitance, has the estimator in full).
//
// With the null boundary and a convex shape a path leaves at most once, so a lane keeps its one (key, w) in registers and the wave deposits
// ONCE, after the event loop, with all 64 lanes converged.  The event loop itself needs no wave-uniform trip count for the deposit; it keeps
// K_fluence's form so that the walk is the same code.
#pragma once
#include "mer_fluence.hpp"          // wave_sum_f64 and, through mer_ptracer.hpp, emit_ray and the bounds PT_* of a light path

namespace mer {

enum { CHK_EXITANCE = 34 };         // bounds-check kind of the sums of an exitance map (mer_device.hpp numbers the others from 1, mer_sdf_build.hip has 32, 33)

// the map of one mer_exitance handle on the device: sums = double[frames][faces][res_v][res_u][3], totals = double[16] (mer.h)
struct ExitanceMap {
    double *sums, *totals;
    unsigned long long *chk;
    int32_t res_u, res_v, faces, frames;
    float t_min, t_bin, cos_min;
    __host__ __device__ uint64_t n_keys() const { return (uint64_t) frames * (uint64_t) faces * (uint64_t) res_v * (uint64_t) res_u; }
};

// floor(f * res) clamped into 0 ... res - 1 (a NaN ends as 0): the point is on the boundary by construction, so it is never dropped
__device__ __forceinline__ uint32_t exitance_index(float f, int32_t res) {
    return (uint32_t) fminf(fmaxf(floorf(f * (float) res), 0.0f), (float) (res - 1));
}

// the cell (face, iv, iu) of the surface point x as one index face * res_v * res_u + iv * res_u + iu.  Cube: the face by shape_normal's rule
// (the axis whose plane the point is relatively closest to, the sign by the side of the centre), face = 2 axis + (sign > 0), u = axis + 1,
// v = axis + 2 (mod 3).  Sphere: one face of equal-area cells, iv from (1 + q.z) / 2, iu from the azimuth / 2 pi wrapped into [0, 1).
__device__ __forceinline__ uint32_t exitance_cell(const mer_scene_desc &S, const ExitanceMap &M, f3 x) {
    if (S.boundary == MER_BOUNDARY_SPHERE) {
        const f3 q = normalize(f3(x.x - S.sph_center[0], x.y - S.sph_center[1], x.z - S.sph_center[2]));
        float a = atan2f(q.y, q.x) * (0.5f / MER_PI);
        if (a < 0.0f) a += 1.0f;
        return exitance_index(0.5f * (1.0f + q.z), M.res_v) * (uint32_t) M.res_u + exitance_index(a, M.res_u);
    }
    float best = -1.0f; int axis = 0, pos = 1;
    const float xx[3] = {x.x, x.y, x.z};
#pragma unroll
    for (int i = 0; i < 3; ++i) {
        const float c = 0.5f * (S.bmin[i] + S.bmax[i]), hsz = 0.5f * (S.bmax[i] - S.bmin[i]);
        const float r = fabsf(xx[i] - c) / hsz;
        if (r > best) { best = r; axis = i; pos = xx[i] >= c ? 1 : 0; }
    }
    const int ua = axis == 2 ? 0 : axis + 1, va = axis == 0 ? 2 : axis - 1;          // (axis + 1) % 3, (axis + 2) % 3
    const float xu = ua == 0 ? x.x : (ua == 1 ? x.y : x.z), xv = va == 0 ? x.x : (va == 1 ? x.y : x.z);
    const uint32_t iu = exitance_index((xu - S.bmin[ua]) / (S.bmax[ua] - S.bmin[ua]), M.res_u);
    const uint32_t iv = exitance_index((xv - S.bmin[va]) / (S.bmax[va] - S.bmin[va]), M.res_v);
    return ((uint32_t) (2 * axis + pos) * (uint32_t) M.res_v + iv) * (uint32_t) M.res_u + iu;
}

// Every lane of the wave calls this together, once per path (dep = the lane has an exit w for `key`): the ballot / shuffle merge of
// fluence_deposit (mer_fluence.hpp) over the map's keys.  Measured against one lane, three atomics (the exitance map; 4.2 M paths):
// 45 x the speed when a collimated beam through a clear cube puts every exit into one cell (3.3 against 151 ms), 4.5 x in a scattering medium
// (sigma_s 2) on a 64 x 64 map, 3.6 x on 4 x 4: the beam's cell still takes most exits of a wave.  The merge stays; the other form is deleted.
__device__ __forceinline__ void exitance_deposit(const ExitanceMap &M, bool dep, uint32_t key, f3 w) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(dep);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const uint32_t lk = (uint32_t) __shfl((int) key, leader, 64);
        const bool same = dep && key == lk;
        const unsigned long long m = __ballot(same);
        double a = same ? (double) w.x : 0.0, b = same ? (double) w.y : 0.0, c = same ? (double) w.z : 0.0;
        if (m & (m - 1ULL)) { a = wave_sum_f64(a); b = wave_sum_f64(b); c = wave_sum_f64(c); }
        if (lane == leader) {
            double *dst = M.sums + MER_CHK(M.chk, CHK_EXITANCE, (uint64_t) lk * 3u, M.n_keys() * 3u - 2u);
            atomicAdd(dst, a); atomicAdd(dst + 1, b); atomicAdd(dst + 2, c);
        }
        todo &= ~m;
    }
}

// K_exitance: light path j = work id `first + j` of the shard, as K_fluence has it
template <bool CURVED, int RIF, int STEPPER, int SIGMA>
__global__ void __launch_bounds__(PT_BLOCK) exitance_kernel(const Params P, const ExitanceMap M, uint64_t first, uint32_t count) {
    const mer_scene_desc &S = P.sc;
    const uint32_t j = blockIdx.x * PT_BLOCK + threadIdx.x;
    LaneCounters C; C.clear();
    int x = 0, y = 0; uint32_t sample = 0;
    const bool live = j < count && decode_work(P, first + j, x, y, sample);        // a work id of a partial tile may fall outside the image
    Rng rng; rng.seed(P.seed, live ? (uint32_t) (y * S.width + x) : 0u, sample);
    const int maxDepth = S.max_depth;
    f3 ps(0, 0, 0), dcur(0, 0, 1), power(0, 0, 0), T(1, 1, 1);
    int depth = 1;
    int alive = 0;                                           // int: a flag that lives across the event loop (compiler note 1)
    bool entering = false;                                   // the next segment starts on the boundary (ray.mint = Epsilon)
    f3 escaped(0, 0, 0);                                     // a path escapes once
    int exited = 0, miss = 0;                                // ... through the boundary at xe heading de after the path length plen, or without meeting the shape
    f3 xe(0, 0, 0), de(0, 0, 1);
    uint32_t ended = 0;
    float plen = 0.0f;                                       // the optical path length, accumulated in float32 as K_fluence does for a time-resolved grid
    // Russian roulette at the end of every loop trip of process() (particleproc.cpp:258-267): q = min(max throughput, 0.95), no eta^2
    auto roulette = [&]() -> bool {
        if (depth++ >= S.rr_depth) {
            const float q = fminf(max3(T), 0.95f);
            if (rng.next1D() >= q) return false;
            T = T / q;
        }
        return true;
    };
    if (live) {
        C.paths++;
        // ---- emission (Scene::sampleEmitterRay), as K_ptracer
        float pk; const int k = emitter_select(P.points, P.n_point, rng, 3, pk);
        power = emit_ray(P, k, rng, ps, dcur);
        alive = !is_zero(power);
        if (alive && !inside_shape(S, ps)) {
            // an emitter outside the shape: the ray meets the null boundary (a surface vertex: one depth) or nothing
            alive = 0;
            if (depth <= maxDepth || maxDepth < 0) {
                const float tIn = intersect_shape(S, ps, dcur, 0.0f, MER_INF);
                if (tIn >= 0) { plen += tIn; ps = ps + dcur * tIn; entering = true; alive = roulette(); }      // the exterior leg: index 1
                else { escaped = power; miss = 1; }          // the emitted ray misses the shape: no exit point
            }
        }
    }

    Walk<CURVED, RIF, STEPPER, SIGMA> W;
    for (int event = 0; event < PT_MAX_EVENTS; ++event) {
        if (!__ballot(alive != 0)) break;                    // wave-uniform, as K_fluence: the wave leaves when its last path has ended
        if (alive) {
            alive = 0;
            if (!is_zero(T) && (depth <= maxDepth || maxDepth < 0)) {
                // ---- free flight (Medium::sampleDistance over [0, its.t]; curved: to the collision or the boundary)
                float itsT = 0.0f;
                if (!CURVED) itsT = intersect_shape(S, ps, dcur, entering ? MER_EPSILON : 0.0f, MER_INF);
                entering = false;
                if (!(itsT >= 0)) { escaped = T * power; exited = 1; xe = ps; de = dcur; }      // on the boundary, heading out
                else {
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
                    if (ev == EV_REAL) {
                        MRec m;
                        finish_free_flight(P, C, W, true, sigma, m);
                        if (SIGMA == MER_SIGMA_HOMOGENEOUS && m.p.x == ps.x && m.p.y == ps.y && m.p.z == ps.z) ended++;       // no forward progress
                        else {
                            C.real++;
                            plen += CURVED ? m.opticalLength : m.t * S.rif_const;
                            T = T * (m.sigmaS * m.transmittance / m.pdfSuccess);
                            const f3 wi = CURVED ? normalize(-m.d) : -W.v;
                            ps = m.p;
                            // ---- phase-function sampling, then the roulette
                            const float p2x = rng.next1D(), p2y = rng.next1D();
                            f3 wo; float phasePdf;
                            const float pw = phase_sample(S.phase, S.g, wi, p2x, p2y, wo, phasePdf);
                            T = T * pw;
                            dcur = wo;
                            alive = roulette();
                        }
                    } else if (ev == EV_GATE_FAIL) ended++;  // the step budget ran out, or the start gate of a B-spline field refused the point
                    else {
                        // the path left the convex shape.  The walk's own state is read as it stands: finish_free_flight(..., false, ...)
                        // would fetch the RIF on a curved ray and count it
                        escaped = T * power; exited = 1;
                        if (CURVED) {
                            // W.pos() is the last point inside; the shape is met again along the momentum (the re-hit of the dielectric
                            // boundary, mer_wavefront.hpp).  The piece x0 -> x, shorter than one stepsize, adds nothing to the path length.
                            const f3 x0 = W.pos();
                            de = normalize(W.v);
                            const float t = intersect_shape(S, x0, de, 0.0f, MER_INF);
                            xe = t >= 0 ? x0 + de * t : x0;
                            plen += W.opt;
                        } else { xe = ps + dcur * itsT; de = dcur; plen += itsT * S.rif_const; }
                    }
                }
            }
        }
    }
    if (alive) ended++;                                      // PT_MAX_EVENTS

    // ---- the one deposit of the path: cone (tested first), window, cell.  Every lane of the wave gets here.
    double rejected[3] = {0.0, 0.0, 0.0}, late[3] = {0.0, 0.0, 0.0}, missed[3] = {0.0, 0.0, 0.0};
    bool dep = false; uint32_t key = 0;
    if (miss) { missed[0] = (double) escaped.x; missed[1] = (double) escaped.y; missed[2] = (double) escaped.z; }
    if (exited) {
        dep = true;
        if (M.cos_min > 0.0f && dot(de, shape_normal(S, xe)) < M.cos_min) {
            dep = false; rejected[0] = (double) escaped.x; rejected[1] = (double) escaped.y; rejected[2] = (double) escaped.z;
        } else if (M.t_bin > 0.0f) {
            const float b = floorf((plen - M.t_min) / M.t_bin);
            if (b >= 0.0f && b < (float) M.frames) key = (uint32_t) b * (uint32_t) (M.faces * M.res_v * M.res_u);      // the key stays below 2^27
            else { dep = false; late[0] = (double) escaped.x; late[1] = (double) escaped.y; late[2] = (double) escaped.z; }
        }
        if (dep) key += exitance_cell(S, M, xe);
    }
    exitance_deposit(M, dep, key, escaped);

    // totals and counters: one wave-aggregated flush each
    const double tot[15] = {(double) wave_sum(C.paths), wave_sum_f64((double) escaped.x), wave_sum_f64((double) escaped.y), wave_sum_f64((double) escaped.z),
                            wave_sum_f64(missed[0]), wave_sum_f64(missed[1]), wave_sum_f64(missed[2]), (double) wave_sum(ended),
                            wave_sum_f64(late[0]), wave_sum_f64(late[1]), wave_sum_f64(late[2]),
                            wave_sum_f64(rejected[0]), wave_sum_f64(rejected[1]), wave_sum_f64(rejected[2]), (double) wave_sum(dep ? 1u : 0u)};
    const uint32_t sums[8] = {wave_sum(C.paths), wave_sum(C.steps), wave_sum(C.rif_evals), wave_sum(C.tentative), wave_sum(C.real), wave_sum(C.segments),
                              wave_sum(C.nee), wave_sum(C.marched)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 15; q++) if (tot[q] != 0.0) atomicAdd(M.totals + q, tot[q]);
        unsigned long long *dst = P.counters + (size_t) (blockIdx.x % MER_COUNTER_REPLICAS) * MER_C_COUNT;
#pragma unroll
        for (int q = 0; q < 7; q++) if (sums[q]) atomicAdd(dst + q, (unsigned long long) sums[q]);
        if (sums[7]) atomicAdd(dst + MER_C_ACTIVE_LANES, (unsigned long long) sums[7]);
    }
}

}  // namespace mer
