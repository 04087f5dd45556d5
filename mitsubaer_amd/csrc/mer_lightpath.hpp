// mer_lightpath.hpp -- the walk of one light path, shared by every kernel that records something from light paths: K_ptracer (mer_ptracer.hpp),
// K_fluence (mer_fluence.hpp), K_fluence_track (mer_fluence_track.hpp), K_exitance (mer_exitance.hpp) and K_detect / K_replay
// (mer_sensitivity.hpp).  ParticleTracer::process
// (src/librender/particleproc.cpp:107-270) restricted to one convex index-matched shape with an interior medium: work id and sampler key,
// emitter_select, emit_ray, the entry into the shape (one depth for the null boundary), the free flights through Walk, phase_sample, the
// roulette, PT_MAX_EVENTS and PT_STEP_BUDGET.  For one scene, shard and seed the four kernels walk the same paths draw for draw because they
// call the same steps -- the members of LightPath below -- in the same order.  What a kernel keeps to itself is its event-loop skeleton
// (K_ptracer: lane-divergent, with `break`; the others: wave-uniform, so that all 64 lanes meet at the deposit) and what it records.
//
// One lane runs one path.  Every loop has a bound: the path's step budget (PT_STEP_BUDGET march units), PT_MAX_EVENTS scatterings and the
// walk's own caps; the host launches PT_PATHS_PER_LAUNCH (curved rays: PT_PATHS_PER_LAUNCH_CURVED) paths at a time.
#pragma once
#include "mer_walk.hpp"

namespace mer {

#define PT_BLOCK 64
#define PT_PATHS_PER_LAUNCH (1u << 20)       // paths per kernel launch, straight rays (launch_light_paths): no launch runs long (measured: 7 ms)
#define PT_PATHS_PER_LAUNCH_CURVED (1u << 16)   // ... curved rays: one resident wave per SIMD of the chip (measured: 0.7 s with the acoustic example scene)
#define PT_MAX_EVENTS 4096                   // scatterings + boundary crossings of one path (Russian roulette ends paths long before)
#define PT_STEP_BUDGET (1u << 22)            // march units (eikonal steps / tentative collisions) of one path over all its free flights

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

// how LightPath::emit left the path
enum { LP_DEAD = 0,      // it ends before its first flight: no power, or no depth left for the null boundary
       LP_INSIDE,        // the emitter lies inside the shape
       LP_ENTERED,       // the emitter lies outside: the ray met the null boundary after tIn (one depth, the roulette has run: `alive` has its answer)
       LP_MISSED };      // the emitter lies outside and the ray misses the shape

// The state of one light path between its events, and the steps every light-path kernel takes.  W is the caller's Walk<CURVED, RIF, STEPPER, SIGMA>.
template <bool CURVED, int SIGMA>
struct LightPath {
    Rng rng;
    f3 ps, dcur;             // the vertex the next flight starts from and its direction
    f3 power, T;             // the emitted weight and the path's throughput
    int depth, maxDepth;     // maxDepth = the scene's max_depth, read once: a load inside the branches costs K_fluence_track scalar registers (one walk for every light-path kernel)
    int alive;               // int: a flag that lives across the event loop (compiler note 1)
    bool entering;           // the next segment starts on the boundary (ray.mint = Epsilon)

    // Russian roulette at the end of every loop trip of process() (particleproc.cpp:258-267): q = min(max throughput, 0.95), no eta^2.
    // 0: the path ends here.
    __device__ __forceinline__ int roulette(const mer_scene_desc &S) {
        if (depth++ >= S.rr_depth) {
            const float q = fminf(max3(T), 0.95f);
            if (rng.next1D() >= q) return 0;
            T = T / q;
        }
        return 1;
    }

    // ---- the start of a path, in two steps: K_ptracer puts the pixel's unit of weight between them, and keeps its whole path inside the one
    // branch on decode's answer (one branch in decode and a second in the kernel cost its straight homogeneous instance a register and a wave).
    // decode: light path j of the launch = work id `first + j` of the shard = the (pixel, sample index) pair K_gen would enumerate
    // (decode_work); its sampler stream is keyed by that pair.  false: no path -- the work id lies past the launch or, in a partial tile,
    // outside the image; the lane seeds pixel 0, draws nothing and idles (alive = 0) through a wave-uniform loop.
    __device__ __forceinline__ bool decode(const Params &P, LaneCounters &C, uint64_t first, uint32_t count, int &x, int &y) {
        const uint32_t j = blockIdx.x * PT_BLOCK + threadIdx.x;
        return decode_id(P, C, j < count, first + j, x, y);
    }
    // decode_id: the same start from a work id the caller holds (have = false: the lane has none).  K_replay (mer_sensitivity.hpp) reads
    // its ids from the list K_detect wrote, so that a lane re-walks exactly the path that lane of K_detect walked.
    __device__ __forceinline__ bool decode_id(const Params &P, LaneCounters &C, bool have, uint64_t w, int &x, int &y) {
        const mer_scene_desc &S = P.sc;
        uint32_t sample = 0;
        x = 0; y = 0;
        const bool live = have && decode_work(P, w, x, y, sample);        // a work id of a partial tile may fall outside the image
        rng.seed(P.seed, live ? (uint32_t) (y * S.width + x) : 0u, sample);
        ps = f3(0, 0, 0); dcur = f3(0, 0, 1); power = f3(0, 0, 0); T = f3(1, 1, 1);
        depth = 1; maxDepth = S.max_depth; alive = 0; entering = false;
        if (live) C.paths++;
        return live;
    }
    // emit: Scene::sampleEmitterRay -- one emitter by samplingWeight, from a forked stream as emitter_select has it.  An emitter outside the
    // shape: the ray meets the null boundary (a surface vertex: one depth, as in volpath) or nothing; tIn is the exterior leg (index 1), which
    // the caller adds to its path length.
    __device__ __forceinline__ int emit(const Params &P, float &tIn) {
        const mer_scene_desc &S = P.sc;
        tIn = 0.0f;
        float pk; const int k = emitter_select(P.points, P.n_point, rng, 3, pk);
        power = emit_ray(P, k, rng, ps, dcur);
        if (is_zero(power)) return LP_DEAD;
        if (inside_shape(S, ps)) { alive = 1; return LP_INSIDE; }
        if (!(depth <= maxDepth || maxDepth < 0)) return LP_DEAD;
        tIn = intersect_shape(S, ps, dcur, 0.0f, MER_INF);
        if (!(tIn >= 0)) return LP_MISSED;
        ps = ps + dcur * tIn; entering = true;
        alive = roulette(S);
        return LP_ENTERED;
    }

    // the path may take another flight: it still carries weight and has depth left
    __device__ __forceinline__ bool can_fly() const { return !is_zero(T) && (depth <= maxDepth || maxDepth < 0); }

    // straight rays: the distance to the boundary along the flight (below 0: on the boundary, heading out); curved rays walk to it
    __device__ __forceinline__ float boundary_distance(const mer_scene_desc &S) {
        float itsT = 0.0f;
        if (!CURVED) itsT = intersect_shape(S, ps, dcur, entering ? MER_EPSILON : 0.0f, MER_INF);
        entering = false;
        return itsT;
    }

    // ---- free flight (Medium::sampleDistance over [0, its.t]; curved: to the collision or the boundary).  Two steps, because the curved
    // branch of K_fluence_track runs the transitions in a wave-uniform loop of its own between them.
    template <class WalkT>
    __device__ __forceinline__ int begin_flight(const Params &P, LaneCounters &C, WalkT &W, float itsT) {
        C.segments++;
        W.t = 0; W.tmin = 0; W.tmax = 0; W.n0 = 1; W.rem = 0; W.steps_left = 0; W.seg_inf = 0; W.sdens = 0; W.backstep = 0; W.hprev = 0; W.cc.reset();
        return W.begin(P, rng, C, K_FREE, ps, dcur, itsT);
    }
    // EV_REAL: a real collision (sigma is its sigma_t); EV_GATE_FAIL: the step budget ran out, or the start gate of a B-spline field refused
    // the point; anything else: the path left the convex shape (no further surface: process() :187-189)
    template <class WalkT>
    __device__ __forceinline__ int run_flight(const Params &P, LaneCounters &C, WalkT &W, int ev, float &sigma) {
        for (;;) {
            if (ev == EV_NONE) { if (C.marched >= PT_STEP_BUDGET) { ev = EV_GATE_FAIL; break; } ev = W.advance(P, rng, C); }
            else if (ev == EV_ARRIVED) ev = W.on_arrived(P, rng, C, sigma);
            else if (ev == EV_EXITED) ev = EV_FAIL;
            else break;
        }
        return ev;
    }
    // the record of the real collision a flight ended in; false: no forward progress, the path ends
    template <class WalkT>
    __device__ __forceinline__ bool collide(const Params &P, LaneCounters &C, WalkT &W, float sigma, MRec &m) {
        finish_free_flight(P, C, W, true, sigma, m);
        if (SIGMA == MER_SIGMA_HOMOGENEOUS && m.p.x == ps.x && m.p.y == ps.y && m.p.z == ps.z) return false;
        C.real++;
        return true;
    }

    // ---- "the flight reached the boundary", in two steps.  A path whose flight fails leaves with T power times the transmittance /
    // pdfFailure of that flight (process() :190-196).  In a homogeneous medium that factor depends on the flight through its length alone
    // -- strategy_pdfs with the scene's sampling density: what finish_free_flight(..., false, ...) would produce, without its RIF fetch and
    // its counter -- and a path leaves once, so K_fluence and K_fluence_track keep T power and this length across their event loop and apply
    // the factor after it, where the walk's registers are free (inside the loop the second copy of strategy_pdfs cost K_fluence's straight
    // homogeneous instance its fifth wave; K_exitance applies it in place: after its loop it cost the acoustic Verlet instance 36 bytes of
    // scratch).  exit_distance: straight rays, W.dist.  A curved flight fails exactly when its sampled distance passes the
    // boundary, somewhere inside the step that left the shape, but W.dist stops at the last step inside (and one step earlier still after
    // traceTillBoundary's step back): half of the leaving step is added, which removes the error of first order in the stepsize -- what is
    // left of it in the weight is (delta sigma_t x stepsize)^2 / 24.  (Intersecting the shape from the last point inside gives the rest
    // exactly, and costs the curved instances of K_fluence 8 - 12 VGPRs, two of them a wave, and one of K_fluence_track 36 bytes of scratch.)
    template <class WalkT>
    __device__ __forceinline__ float exit_distance(const WalkT &W) const {
        if (SIGMA != MER_SIGMA_HOMOGENEOUS) return 0.0f;
        return CURVED ? W.dist + (W.seg_inf ? 1.5f : 0.5f) * W.hprev : W.dist;
    }
    // w *= transmittance / pdfFailure at the length d of the failed flight (below 0: the path did not leave; 0 weighs 1 exactly).  The factor
    // is identically 1, and skipped by a scene-uniform test, when one exponential of the medium's own sigma_t draws every flight: the
    // three sigma_t equal, medium_sampling_weight == 1 and no manual density; a gridded sigma_t has transmittance = pdfFailure.  A
    // transmittance that underflowed to 0 over a pdfFailure of 0 weighs 0.
    static __device__ __forceinline__ void weigh_exit(const Params &P, float d, f3 &w) {
        if (SIGMA != MER_SIGMA_HOMOGENEOUS) return;
        const bool analog = P.sigT.x == P.sigT.y && P.sigT.y == P.sigT.z && P.medium_sampling_weight == 1.0f && P.sc.strategy != MER_STRATEGY_MANUAL;
        if (analog || !(d >= 0.0f)) return;
        f3 tr; float pdfSuccess, pdfFailure;
        strategy_pdfs(P, d, P.sampling_density, tr, pdfSuccess, pdfFailure);
        w = pdfFailure > 0.0f ? w * (tr / pdfFailure) : f3(0, 0, 0);
    }

    // ---- scattering, in two steps (K_ptracer connects the vertex to the sensor between them).  arrive: the throughput at the vertex
    // (process() :174) and the direction the path came from; scatter: phase-function sampling (EImportance; hg and isotropic are symmetric),
    // then the roulette.
    template <class WalkT>
    __device__ __forceinline__ f3 arrive(const WalkT &W, const MRec &m) {
        T = T * (m.sigmaS * m.transmittance / m.pdfSuccess);
        const f3 wi = CURVED ? normalize(-m.d) : -W.v;
        ps = m.p;
        return wi;
    }
    __device__ __forceinline__ void scatter(const mer_scene_desc &S, f3 wi) {
        const float p2x = rng.next1D(), p2y = rng.next1D();
        f3 wo; float phasePdf;
        const float pw = phase_sample(S.phase, S.g, wi, p2x, p2y, wo, phasePdf);
        T = T * pw;
        dcur = wo;
        alive = roulette(S);
    }
};

// counters: one wave-aggregated flush (every lane of the wave calls this together)
__device__ __forceinline__ void flush_counters(const Params &P, const LaneCounters &C) {
    const uint32_t sums[8] = {wave_sum(C.paths), wave_sum(C.steps), wave_sum(C.rif_evals), wave_sum(C.tentative), wave_sum(C.real), wave_sum(C.segments),
                              wave_sum(C.nee), wave_sum(C.marched)};
    if ((threadIdx.x & 63) == 0) {
        unsigned long long *dst = P.counters + (size_t) (blockIdx.x % MER_COUNTER_REPLICAS) * MER_C_COUNT;
#pragma unroll
        for (int q = 0; q < 7; q++) if (sums[q]) atomicAdd(dst + q, (unsigned long long) sums[q]);
        if (sums[7]) atomicAdd(dst + MER_C_ACTIVE_LANES, (unsigned long long) sums[7]);
    }
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// Every lane of the wave calls this together (dep = the lane has a deposit w for `key`, one of the n_keys RGB triples of `sums`).  The lanes
// that deposit into the first pending lane's key are found with a ballot, their three channels are summed over the wave in float64, that
// first lane issues the three atomics, and the group leaves the pending mask: at most 64 trips, one per distinct key.  A group of one skips
// the sums.  Measured against one lane, three atomics, at each site that deposits (DESIGN.md has every A/B):
//   the fluence grid, collisions: 1.75 x the paths/s of the laser example on a 32^3 grid, 5.1 x on 8^3, a tie on 128^3;
//   the time-resolved grid, key = frame * n_cells + cell (32^3, 1 / 16 / 100 frames): a tie on the acoustic field, where the walk dominates, and
//     on the homogeneous medium a tie when the window holds a tenth of the deposits, 1.7 - 1.8 x when it holds nearly all;
//   the track-length grid, one piece per lane per trip: 6.6 x on the grey laser scene at 8^3, 4.3 x at 32^3, 3.2 x at 128^3 -- spread-out flights
//     still share cells along the beam -- and 1.1 x in the acoustic field;
//   the exitance map, once per path (4.2 M paths): 45 x when a collimated beam through a clear cube puts every exit into one cell (3.3 against
//     151 ms), 4.5 x in a scattering medium (sigma_s 2) on a 64 x 64 map, 3.6 x on 4 x 4: the beam's cell still takes most exits of a wave.
__device__ __forceinline__ void wave_deposit(double *sums, unsigned long long *chk, int chk_kind, uint64_t n_keys, bool dep, uint32_t key, f3 w) {
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
            double *dst = sums + MER_CHK(chk, chk_kind, (uint64_t) lk * 3u, n_keys * 3u - 2u);
            atomicAdd(dst, a); atomicAdd(dst + 1, b); atomicAdd(dst + 2, c);
        }
        todo &= ~m;
    }
}

// The frequency-domain recorders (mer.h, mer_fluence_fd_create): (cos, sin) of phi = k l for the wavenumber k (float64) and the optical path
// length l (float32).  phi is reduced to [-pi, pi] in float64 and rounded to float32 once -- pi 2^-24 -- and the float32 functions add their
// 2 ulp: 2^-21 absolute at most, whatever the size of phi.  The pair is then brought to unit modulus in float64 (one Newton step of
// 1 / sqrt(c^2 + s^2) from 1: c^2 + s^2 is within 2^-21 of 1, so what is left is below 1e-12).  That takes out the radial part of the
// error -- the exact pair lies on the unit circle, so the projection brings the computed one no further from it -- and lets no deposit
// weigh more than its w: the modulus of a cell never exceeds its steady sum.  k = 0: phi = 0 and (1, 0) exactly.
__device__ __forceinline__ void fd_phase(double k, float l, double &c, double &s) {
    const double phi = k * (double) l;
    const double r = phi - rint(phi * 0.15915494309189535) * 6.283185307179586;
    float sf, cf;
    sincosf((float) r, &sf, &cf);
    c = (double) cf; s = (double) sf;
    const double f = 1.5 - 0.5 * (c * c + s * s);
    c *= f; s *= f;
}
// wave_deposit for a deposit that is float64 already: the same merge of equal keys over the wave
__device__ __forceinline__ void wave_deposit_f64(double *sums, unsigned long long *chk, int chk_kind, uint64_t n_keys, bool dep, uint32_t key, double x, double y, double z) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(dep);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const uint32_t lk = (uint32_t) __shfl((int) key, leader, 64);
        const bool same = dep && key == lk;
        const unsigned long long m = __ballot(same);
        double a = same ? x : 0.0, b = same ? y : 0.0, c = same ? z : 0.0;
        if (m & (m - 1ULL)) { a = wave_sum_f64(a); b = wave_sum_f64(b); c = wave_sum_f64(c); }
        if (lane == leader) {
            double *dst = sums + MER_CHK(chk, chk_kind, (uint64_t) lk * 3u, n_keys * 3u - 2u);
            atomicAdd(dst, a); atomicAdd(dst + 1, b); atomicAdd(dst + 2, c);
        }
        todo &= ~m;
    }
}
// Every lane of the wave calls this together: the deposit w of `cell` (one of n_cells) into the 2 n_freq planes of `sums`, plane 2 j + part at
// key (2 j + part) * n_cells + cell, w cos(k_j l) into the real part and w sin(k_j l) into the imaginary one, the products in float64.  The
// loop over the planes is wave-uniform (n_freq and k_j are scalars), every plane is merged over the wave as wave_deposit merges, and the
// imaginary plane of k_j = 0 is never touched.
__device__ __forceinline__ void wave_deposit_fd(double *sums, unsigned long long *chk, int chk_kind, uint32_t n_cells, const double *wavenumber, int n_freq,
                                                bool dep, uint32_t cell, f3 w, float l) {
    const uint64_t n_keys = (uint64_t) (2 * n_freq) * n_cells;
    const double wx = (double) w.x, wy = (double) w.y, wz = (double) w.z;
    // the wavenumbers are read through the constant address space: written before the launch and by no kernel, so the load is scalar and
    // waits for nothing.  As a plain global load it is a vector load whose s_waitcnt vmcnt(0) also waits for the atomics of the plane
    // before it (measured: 13.5 against 5.8 ms for one plane of the laser example's grid)
    typedef const double __attribute__((address_space(4))) *ConstantF64;
    const ConstantF64 wn = (ConstantF64) (uintptr_t) wavenumber;
    for (int j = 0; j < n_freq; ++j) {
        const double k = wn[j];
        double c, s;
        fd_phase(k, l, c, s);
        wave_deposit_f64(sums, chk, chk_kind, n_keys, dep, (uint32_t) (2 * j) * n_cells + cell, wx * c, wy * c, wz * c);
        if (k != 0.0) wave_deposit_f64(sums, chk, chk_kind, n_keys, dep, (uint32_t) (2 * j + 1) * n_cells + cell, wx * s, wy * s, wz * s);
    }
}

}  // namespace mer
