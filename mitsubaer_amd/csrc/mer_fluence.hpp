// mer_fluence.hpp -- the fluence inside the medium as a voxel grid, recorded from light paths (mer_render_fluence): a grid of the reference's
// `fluencemeter` probes (src/sensors/fluencemeter.cpp:40-41, driven by `ptracer`) instead of one probe per render.
//
// A light path is exactly the one K_ptracer (mer_ptracer.hpp) walks for the same scene, shard and seed -- work id and sampler key, emitter_select,
// emit_ray, the entry into the shape (one depth for the null boundary), the free flights, phase_sample, the roulette, PT_MAX_EVENTS and
// PT_STEP_BUDGET -- without the sensor connection.  Every real collision the loop reaches is a collision-estimator sample of the fluence:
// w = T power (transmittance / pdfSuccess), taken before T is multiplied by the albedo, goes into the cell that holds the collision point
// (mer.h, mer_render_fluence, has the estimator in full).
//
// One lane runs one path, as in K_ptracer, but the event loop is WAVE-UNIFORM: it runs while any lane of the wave has a live path, and a lane
// whose path has ended idles through the body.  All 64 lanes therefore meet at the single deposit site at the end of the body, outside the
// lane-dependent free-flight loop, where fluence_deposit merges the deposits of equal cells over the wave before it touches memory.
//
// TIMED (a handle of mer_fluence_time_create): the same walk, draw for draw, that also carries the light tracer's optical path length `plen`
// (float32: the exterior leg at index 1, then m.opticalLength or m.t * rif_const per free flight) and bins every deposit by it:
// frame = floorf((plen - t_min) / t_bin), key = frame * n_cells + cell.  The window is the handle's own; the film fields stay ignored.
#pragma once
#include "mer_ptracer.hpp"          // emit_ray and the bounds PT_* of a light path; the Connector it brings along is not instantiated here

namespace mer {

// the grid of one mer_fluence handle on the device: sums = double[nz][ny][nx][3], totals = double[8] (mer.h); a time-resolved handle:
// sums = double[frames][nz][ny][nx][3], n_keys() = frames * n_cells of them (at most 2^27), totals = double[12].  The steady-state
// kernels read none of the fields after bmax.
struct FluenceGrid {
    double *sums, *totals;
    unsigned long long *chk;
    uint64_t n_cells;
    int32_t res[3];
    float bmin[3], bmax[3];
    int32_t frames;
    float t_min, t_bin;
    __host__ __device__ uint64_t n_keys() const { return (uint64_t) frames * n_cells; }
};

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// the cell of p: per axis floor((p - bmin) / (bmax - bmin) * res), half-open; false outside the box (and for a p that is not a number)
__device__ __forceinline__ bool fluence_cell(const FluenceGrid &G, f3 p, uint32_t &cell) {
    const float fx = floorf((p.x - G.bmin[0]) / (G.bmax[0] - G.bmin[0]) * (float) G.res[0]);
    const float fy = floorf((p.y - G.bmin[1]) / (G.bmax[1] - G.bmin[1]) * (float) G.res[1]);
    const float fz = floorf((p.z - G.bmin[2]) / (G.bmax[2] - G.bmin[2]) * (float) G.res[2]);
    cell = 0;
    if (!(fx >= 0 && fx < (float) G.res[0] && fy >= 0 && fy < (float) G.res[1] && fz >= 0 && fz < (float) G.res[2])) return false;
    cell = ((uint32_t) fz * (uint32_t) G.res[1] + (uint32_t) fy) * (uint32_t) G.res[0] + (uint32_t) fx;      // at most 2^27 cells
    return true;
}

// Every lane of the wave calls this together (dep = the lane has a deposit w for `cell`).  The lanes that deposit into the first pending
// lane's cell are found with a ballot, their three channels are summed over the wave in float64, that first lane issues the three atomics,
// and the group leaves the pending mask: at most 64 trips, one per distinct cell.  A group of one skips the sums.
// Measured against one lane, three atomics (the fluence grid): 1.75 x the paths/s of the laser example on a 32^3 grid, 5.1 x on 8^3, a tie on 128^3.
// TIMED: `cell` is the key frame * n_cells + cell and the extent is the time-resolved grid's.  With frames the keys of a wave spread further, so
// the A/B was repeated (the time-resolved grid; 32^3, 1 / 16 / 100 frames): a tie on the acoustic field, where the walk dominates, and on
// the homogeneous medium a tie when the window holds a tenth of the deposits, 1.7 - 1.8 x when it holds nearly all.  The merge stays here too.
template <bool TIMED>
__device__ __forceinline__ void fluence_deposit(const FluenceGrid &G, bool dep, uint32_t cell, f3 w) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(dep);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const uint32_t lc = (uint32_t) __shfl((int) cell, leader, 64);
        const bool same = dep && cell == lc;
        const unsigned long long m = __ballot(same);
        double a = same ? (double) w.x : 0.0, b = same ? (double) w.y : 0.0, c = same ? (double) w.z : 0.0;
        if (m & (m - 1ULL)) { a = wave_sum_f64(a); b = wave_sum_f64(b); c = wave_sum_f64(c); }
        if (lane == leader) {
            double *dst = G.sums + MER_CHK(G.chk, CHK_FLUENCE, (uint64_t) lc * 3u, (TIMED ? G.n_keys() : G.n_cells) * 3u - 2u);
            atomicAdd(dst, a); atomicAdd(dst + 1, b); atomicAdd(dst + 2, c);
        }
        todo &= ~m;
    }
}

// K_fluence: light path j = work id `first + j` of the shard, as K_ptracer has it
template <bool CURVED, int RIF, int STEPPER, int SIGMA, bool TIMED>
__global__ void __launch_bounds__(PT_BLOCK) fluence_kernel(const Params P, const FluenceGrid G, uint64_t first, uint32_t count) {
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
    double dropped[3] = {0.0, 0.0, 0.0};
    uint32_t ended = 0;
    float plen = 0.0f;                                       // TIMED: the optical path length, accumulated in float32 as K_ptracer does under a TRANSIENT film
    double late[3] = {0.0, 0.0, 0.0};                        // TIMED: the weight of deposits inside the box but outside the time window
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
                if (tIn >= 0) { if (TIMED) plen += tIn; ps = ps + dcur * tIn; entering = true; alive = roulette(); }      // the exterior leg: index 1
                else escaped = power;                        // the emitted ray misses the shape
            }
        }
    }

    Walk<CURVED, RIF, STEPPER, SIGMA> W;
    for (int event = 0; event < PT_MAX_EVENTS; ++event) {
        if (!__ballot(alive != 0)) break;                    // wave-uniform: the wave leaves when its last path has ended
        bool dep = false; uint32_t cell = 0; f3 w(0, 0, 0);
        if (alive) {
            alive = 0;
            if (!is_zero(T) && (depth <= maxDepth || maxDepth < 0)) {
                // ---- free flight (Medium::sampleDistance over [0, its.t]; curved: to the collision or the boundary)
                float itsT = 0.0f;
                if (!CURVED) itsT = intersect_shape(S, ps, dcur, entering ? MER_EPSILON : 0.0f, MER_INF);
                entering = false;
                if (!(itsT >= 0)) escaped = T * power;       // on the boundary, heading out
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
                            // ---- the deposit: before the albedo
                            w = T * power * (m.transmittance / m.pdfSuccess);
                            dep = fluence_cell(G, m.p, cell);
                            if (!dep) { dropped[0] += (double) w.x; dropped[1] += (double) w.y; dropped[2] += (double) w.z; }
                            if (TIMED) {
                                plen += CURVED ? m.opticalLength : m.t * S.rif_const;
                                if (dep) {
                                    const float b = floorf((plen - G.t_min) / G.t_bin);                  // film_contribute's bin
                                    if (b >= 0.0f && b < (float) G.frames) cell += (uint32_t) b * (uint32_t) G.n_cells;      // the key, below 2^27
                                    else { dep = false; late[0] += (double) w.x; late[1] += (double) w.y; late[2] += (double) w.z; }
                                }
                            }
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
                    else escaped = T * power;                // the path left the convex shape
                }
            }
        }
        fluence_deposit<TIMED>(G, dep, cell, w);
    }
    if (alive) ended++;                                      // PT_MAX_EVENTS

    // totals and counters: one wave-aggregated flush each (every lane of the wave gets here)
    const double tot[8] = {(double) wave_sum(C.paths), wave_sum_f64((double) escaped.x), wave_sum_f64((double) escaped.y), wave_sum_f64((double) escaped.z),
                           wave_sum_f64(dropped[0]), wave_sum_f64(dropped[1]), wave_sum_f64(dropped[2]), (double) wave_sum(ended)};
    const uint32_t sums[8] = {wave_sum(C.paths), wave_sum(C.steps), wave_sum(C.rif_evals), wave_sum(C.tentative), wave_sum(C.real), wave_sum(C.segments),
                              wave_sum(C.nee), wave_sum(C.marched)};
    // out of the window: per lane and flushed once per wave like the other totals -- as one more key of the grid it would be a single
    // address that most deposits of a scene whose window starts late hit (measured: 4 x the time of the whole render on the laser example)
    double out_of_window[3] = {0.0, 0.0, 0.0};
    if (TIMED) { out_of_window[0] = wave_sum_f64(late[0]); out_of_window[1] = wave_sum_f64(late[1]); out_of_window[2] = wave_sum_f64(late[2]); }
    if ((threadIdx.x & 63) == 0) {
        if (TIMED) {
#pragma unroll
            for (int q = 0; q < 3; q++) if (out_of_window[q] != 0.0) atomicAdd(G.totals + 8 + q, out_of_window[q]);
        }
#pragma unroll
        for (int q = 0; q < 8; q++) if (tot[q] != 0.0) atomicAdd(G.totals + q, tot[q]);
        unsigned long long *dst = P.counters + (size_t) (blockIdx.x % MER_COUNTER_REPLICAS) * MER_C_COUNT;
#pragma unroll
        for (int q = 0; q < 7; q++) if (sums[q]) atomicAdd(dst + q, (unsigned long long) sums[q]);
        if (sums[7]) atomicAdd(dst + MER_C_ACTIVE_LANES, (unsigned long long) sums[7]);
    }
}

}  // namespace mer
