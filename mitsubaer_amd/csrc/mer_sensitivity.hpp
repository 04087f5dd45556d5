// mer_sensitivity.hpp -- which part of the medium the detected light travelled through: the absorption sensitivity (Jacobian, photon-
// measurement density function) of one detector on the boundary, as a voxel grid (mer_render_sensitivity; mer.h has the estimator in full).
//
// A path's weight at the detector is known only when it leaves, so a launch chunk runs in two passes over the SAME paths -- the sampler
// stream is keyed by the work id, so a path walks the same way whenever it is walked:
//   K_detect  the exit-recording walk of K_exitance (exit_walk below) without a map.  A lane whose exit passes the detector --
//             cone, gate and cell window, in K_exitance's own expressions -- appends (work id, w) to the context's detected-path list.
//   K_replay  one lane per list record, so its waves are full whatever fraction of the paths is detected.  It re-walks the path in the
//             wave-uniform skeleton of K_fluence_track (mer_fluence_track.hpp) and deposits w x length for the piece of every free flight
//             inside each cell, cut as the track-length grid cuts them.  At the replayed exit it compares the w it recomputed with the
//             recorded one, bit for bit, and counts the disagreements: 0 says the two passes walked the same paths.
// An array of detectors and gates (mer_sensitivity_array_create) costs the same two passes: a path leaves through one raster cell at one
// path length, so it belongs to at most one measurement m.  K_detect records m with the path, K_replay offsets its keys by it and, with
// `scatter`, also deposits w at every scattering collision: the scattering grids K.
#pragma once
#include "mer_exitance.hpp"         // ExitanceMap, exitance_cell
#include "mer_fluence_track.hpp"    // FluenceGrid, fluence_cell, TrackDDA

namespace mer {

// the detected-path list of a context: SoA, so that the lanes of a wave write (and K_replay's read) adjacent words.  id = the work id less
// the launch's `first`, m = the measurement (detector of the array x gate) the path belongs to.  cap = the paths of one launch chunk: the
// list cannot overflow.  One pointer, DETECT_HEAD words whose first is the count, then the five arrays of cap words; the kernels form the
// arrays' addresses themselves: with a pointer per array, and a whole ExitanceMap in the detector, four K_detect instances had 36 bytes of
// scratch (SGPR pressure from the kernel arguments).
#define DETECT_HEAD 64
struct DetectList {
    uint32_t *count;
    uint32_t cap;
    unsigned long long *chk;
    __device__ __forceinline__ uint32_t *id() const { return count + DETECT_HEAD; }
    __device__ __forceinline__ float *w(int c) const { return (float *) (count + DETECT_HEAD + (size_t) (c + 1) * cap); }
    __device__ __forceinline__ uint32_t *m() const { return count + DETECT_HEAD + (size_t) 4 * cap; }
};

// the detectors of a mer_sensitivity handle: the raster, the window, the cone and the gates; one detector is bin_u x bin_v raster cells of
// the window (bins = bin_u | bin_v << 16; mer_sensitivity_create: the whole window), gate g the paths with floorf((l - t_min) / t_bin) == g
struct Detector {
    int32_t res_u, res_v, face, iu0, iu1, iv0, iv1;
    float cos_min, t_min, t_bin;
    uint32_t bins;
    int32_t gates;
};

// MEAS_WORDS float64 per measurement behind the totals of a sensitivity Recorder (mer.h, mer_sensitivity_read_array): [0..2] the detected
// weight and [3] the detected paths (K_detect), [4..6] w x the path's scattering collisions (K_replay), [7] 0
#define MEAS_WORDS 8
#define SENS_TOTALS 16

// Every lane of the wave calls this together, as wave_deposit (mer_lightpath.hpp), whose merging of equal keys this is: the lanes with
// dep add (va, vb, vc, n) into meas[m][off ... off + 3]; one group of atomics per distinct m of the wave.
__device__ __forceinline__ void wave_measure(double *meas, unsigned long long *chk, uint32_t n_meas, bool dep, uint32_t m, int off, double va, double vb, double vc, double n) {
    const int lane = threadIdx.x & 63;
    unsigned long long todo = __ballot(dep);
    while (todo) {
        const int leader = __ffsll((long long) todo) - 1;
        const uint32_t lm = (uint32_t) __shfl((int) m, leader, 64);
        const bool same = dep && m == lm;
        const unsigned long long g = __ballot(same);
        double a = same ? va : 0.0, b = same ? vb : 0.0, c = same ? vc : 0.0, d = same ? n : 0.0;
        if (g & (g - 1ULL)) { a = wave_sum_f64(a); b = wave_sum_f64(b); c = wave_sum_f64(c); d = wave_sum_f64(d); }
        if (lane == leader) {
            double *dst = meas + MER_CHK(chk, CHK_SENSITIVITY, (uint64_t) lm, n_meas) * MEAS_WORDS + off;
            if (a != 0.0) atomicAdd(dst, a);
            if (b != 0.0) atomicAdd(dst + 1, b);
            if (c != 0.0) atomicAdd(dst + 2, c);
            if (d != 0.0) atomicAdd(dst + 3, d);
        }
        todo &= ~g;
    }
}

// What the exit-recording walk leaves in a lane
struct ExitRecord {
    f3 escaped;              // a path escapes once
    f3 xe, de;               // ... through the boundary at xe heading de after the path length plen (dexit >= 0)
    float dexit;             // >= 0: the path left through the boundary, after a flight of this length (LightPath::weigh_exit; 0: from the boundary itself)
    uint32_t ended;
    float plen;              // the optical path length, accumulated in float32 as K_exitance does
};

// K_exitance's walk of light path j = blockIdx.x * PT_BLOCK + threadIdx.x of the launch, from its decode to its end, statement for statement
// (exitance_kernel, mer_exitance.hpp, has the comments): the exit it records is the one the exitance map bins.  A copy, not a function the
// two kernels share: with its walk moved into a function K_exitance computes the same but is allocated differently -- 11 of its 14 instances
// change their VGPR count by -9 ... +6 and the B-spline Verlet gridded one falls from 4 waves per SIMD to 3 (sensitivity maps).
// Every lane of the wave returns.
template <bool CURVED, int RIF, int STEPPER, int SIGMA>
__device__ __forceinline__ void exit_walk(const Params &P, LaneCounters &C, uint64_t first, uint32_t count, ExitRecord &R) {
    const mer_scene_desc &S = P.sc;
    LightPath<CURVED, SIGMA> lp;
    f3 escaped(0, 0, 0);
    f3 xe(0, 0, 0), de(0, 0, 1);
    float dexit = -1.0f;
    uint32_t ended = 0;
    float plen = 0.0f;
    int x, y; float tIn;
    const int how = lp.decode(P, C, first, count, x, y) ? lp.emit(P, tIn) : LP_DEAD;
    if (how == LP_ENTERED) plen += tIn;                      // an emitted ray that misses the shape has no exit point: never detected

    Walk<CURVED, RIF, STEPPER, SIGMA> W;
    for (int event = 0; event < PT_MAX_EVENTS; ++event) {
        if (!__ballot(lp.alive != 0)) break;                 // wave-uniform: the wave leaves when its last path has ended
        if (lp.alive) {
            lp.alive = 0;
            if (lp.can_fly()) {
                const float itsT = lp.boundary_distance(S);
                if (!(itsT >= 0)) { escaped = lp.T * lp.power; dexit = 0.0f; xe = lp.ps; de = lp.dcur; }      // on the boundary, heading out
                else {
                    float sigma = 0.0f;
                    const int ev = lp.run_flight(P, C, W, lp.begin_flight(P, C, W, itsT), sigma);
                    if (ev == EV_REAL) {
                        MRec m;
                        if (!lp.collide(P, C, W, sigma, m)) ended++;
                        else {
                            plen += CURVED ? m.opticalLength : m.t * S.rif_const;
                            lp.scatter(S, lp.arrive(W, m));
                        }
                    } else if (ev == EV_GATE_FAIL) ended++;
                    else {
                        escaped = lp.T * lp.power; dexit = lp.exit_distance(W); lp.weigh_exit(P, dexit, escaped);
                        if (CURVED) {
                            const f3 x0 = W.pos();
                            de = normalize(W.v);
                            const float t = intersect_shape(S, x0, de, 0.0f, MER_INF);
                            xe = t >= 0 ? x0 + de * t : x0;
                            plen += W.opt;
                        } else { xe = lp.ps + lp.dcur * itsT; de = lp.dcur; plen += itsT * S.rif_const; }
                    }
                }
            }
        }
    }
    if (lp.alive) ended++;                                   // PT_MAX_EVENTS
    R.escaped = escaped; R.xe = xe; R.de = de; R.dexit = dexit; R.ended = ended; R.plen = plen;
}

// K_detect.  totals (mer.h): [0] paths, [1..3] the detected weight, [7] ended, [8] the detected paths; the measurements follow the
// totals: meas = totals + SENS_TOTALS.
template <bool CURVED, int RIF, int STEPPER, int SIGMA>
__global__ void __launch_bounds__(PT_BLOCK) detect_kernel(const Params P, const Detector D, const DetectList L, double *totals, uint64_t first, uint32_t count) {
    const mer_scene_desc &S = P.sc;
    LaneCounters C; C.clear();
    ExitRecord R;
    exit_walk<CURVED, RIF, STEPPER, SIGMA>(P, C, first, count, R);

    // ---- the detector: cone (tested first), gate, window.  Every lane of the wave gets here.
    bool det = false;
    uint32_t mi = 0;                                         // the measurement: (gate * ndv + dv) * ndu + du
    if (R.dexit >= 0.0f) {
        det = !(D.cos_min > 0.0f && dot(R.de, shape_normal(S, R.xe)) < D.cos_min);
        if (det && D.t_bin > 0.0f) {
            const float b = floorf((R.plen - D.t_min) / D.t_bin);
            det = b >= 0.0f && b < (float) D.gates;
            if (det) mi = (uint32_t) b;
        }
        if (det) {
            ExitanceMap M; M.res_u = D.res_u; M.res_v = D.res_v;         // all that exitance_cell reads of a map
            const uint32_t cell = exitance_cell(S, M, R.xe), row = cell / (uint32_t) D.res_u;
            const int32_t iu = (int32_t) (cell - row * (uint32_t) D.res_u), iv = (int32_t) (row % (uint32_t) D.res_v), face = (int32_t) (row / (uint32_t) D.res_v);
            det = face == D.face && iu >= D.iu0 && iu < D.iu1 && iv >= D.iv0 && iv < D.iv1;
            if (det) {
                const uint32_t bu = D.bins & 0xffffu, bv = D.bins >> 16;
                mi = (mi * ((uint32_t) (D.iv1 - D.iv0) / bv) + (uint32_t) (iv - D.iv0) / bv) * ((uint32_t) (D.iu1 - D.iu0) / bu) + (uint32_t) (iu - D.iu0) / bu;
            }
        }
    }
    const f3 w = det ? R.escaped : f3(0, 0, 0);

    // ---- the append: one ballot and one returning atomic per wave (queue_push's pattern, mer_wavefront.hpp)
    const unsigned long long mask = __ballot(det);
    if (mask) {
        const int lane = threadIdx.x & 63;
        const int leader = __ffsll((long long) mask) - 1;
        uint32_t base = 0;
        if (lane == leader) base = atomicAdd(L.count, (uint32_t) __popcll(mask));
        base = (uint32_t) __shfl((int) base, leader, 64);
        if (det) {
            const uint64_t at = MER_CHK(L.chk, CHK_DETECT_LIST, base + (uint32_t) __popcll(mask & ((1ULL << lane) - 1ULL)), L.cap);
            L.id()[at] = blockIdx.x * PT_BLOCK + threadIdx.x;
            L.w(0)[at] = w.x; L.w(1)[at] = w.y; L.w(2)[at] = w.z;
            L.m()[at] = mi;
        }
        // the measurements: one group of atomics per distinct measurement of the wave
        wave_measure(totals + SENS_TOTALS, L.chk, (uint32_t) D.gates * ((uint32_t) (D.iv1 - D.iv0) / (D.bins >> 16)) * ((uint32_t) (D.iu1 - D.iu0) / (D.bins & 0xffffu)),
                     det, mi, 0, (double) w.x, (double) w.y, (double) w.z, 1.0);
    }

    // totals and counters: one wave-aggregated flush each, as K_exitance has them
    const double tot[6] = {(double) wave_sum(C.paths), wave_sum_f64((double) w.x), wave_sum_f64((double) w.y), wave_sum_f64((double) w.z),
                           (double) wave_sum(R.ended), (double) __popcll(mask)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 4; q++) if (tot[q] != 0.0) atomicAdd(totals + q, tot[q]);
        if (tot[4] != 0.0) atomicAdd(totals + 7, tot[4]);
        if (tot[5] != 0.0) atomicAdd(totals + 8, tot[5]);
    }
    flush_counters(P, C);
}

// K_replay: lane r of the launch re-walks record r of the list (n records; the lanes past its end idle with alive = 0 through every
// wave-uniform loop).  The skeleton is K_fluence_track's; a piece of length l deposits w l, with w the path's recorded weight at the
// detector, whatever the distance sampling: only the integrand of the detected signal depends on sigma_a.  The walk counters are not flushed:
// mer_counters_read reports the detect pass.  totals: [4..6] w x the length outside the box, [9..11] w x the path's length inside the shape
// (summed per lane in float64 from the flight lengths, before any cutting), [12] the replay disagreements.
// The path's measurement m (of n_meas) offsets its keys: the absorption grid J of m has the keys m * n_cells + cell.  scatter: the
// scattering grids K follow the n_meas absorption grids, key (n_meas + m) * n_cells + cell: every real collision the path scatters from
// deposits w into the cell of the collision point (K_fluence's cell); totals [13..15] w per collision outside the box; meas[m][4..6] w x the
// path's collisions, counted before the box test.
// ARRAY = false: the one measurement without a scattering grid of mer_sensitivity_create, whose instances then compile as they did before
// the arrays (with the measurement and the collision registers in every instance two of the 14 lost a wave per SIMD and two gained 36
// bytes of scratch: DESIGN.md, sensitivity maps); the last two arguments are ignored.
template <bool CURVED, int RIF, int STEPPER, int SIGMA, bool ARRAY>
__global__ void __launch_bounds__(PT_BLOCK) replay_kernel(const Params P, const FluenceGrid G, const DetectList L, uint64_t first, uint32_t n,
                                                          uint32_t n_meas_arg, uint32_t scatter_arg) {
    const uint32_t n_meas = ARRAY ? n_meas_arg : 1u, scatter = ARRAY ? scatter_arg : 0u;
    const mer_scene_desc &S = P.sc;
    LaneCounters C; C.clear();
    LightPath<CURVED, SIGMA> lp;
    const uint32_t r = blockIdx.x * PT_BLOCK + threadIdx.x;
    const bool have = r < n;
    uint32_t j = 0, kbase = 0; f3 w(0, 0, 0);
    if (have) {
        const uint64_t at = MER_CHK(L.chk, CHK_DETECT_LIST, r, L.cap);
        j = L.id()[at]; w = f3(L.w(0)[at], L.w(1)[at], L.w(2)[at]);
        if (ARRAY) kbase = L.m()[at] * (uint32_t) G.n_cells;      // at most 2^27 keys
    }
    const uint64_t n_keys = (uint64_t) (1u + scatter) * n_meas * G.n_cells;
    uint32_t collisions = 0, collisions_out = 0;             // scatter: the path's scattering collisions, and those outside the box
    f3 escaped(0, 0, 0);
    float dexit = -1.0f;                                     // the length of the flight that reached the boundary (LightPath::weigh_exit)
    int left = 0;                                            // the replayed path left through the boundary
    double inside = 0.0, outside = 0.0;                      // the path's length inside the shape, and the part of it outside the box
    int x, y; float tIn;
    if (lp.decode_id(P, C, have, first + j, x, y)) (void) lp.emit(P, tIn);

    Walk<CURVED, RIF, STEPPER, SIGMA> W;
    TrackDDA D;
    uint32_t run_cell = 0; float run_l = 0.0f; int run_on = 0;           // CURVED: the lane's run of chords in one cell
    for (int event = 0; event < PT_MAX_EVENTS; ++event) {
        if (!__ballot(lp.alive != 0)) break;
        int ev = EV_FAIL, flight = 0;
        float itsT = 0.0f, sigma = 0.0f;
        const f3 fo = lp.ps, fd = lp.dcur;                   // the flight's start and direction
        if (lp.alive) {
            lp.alive = 0;
            if (lp.can_fly()) {
                itsT = lp.boundary_distance(S);
                if (!(itsT >= 0)) { escaped = lp.T * lp.power; left = 1; }
                else { ev = lp.begin_flight(P, C, W, itsT); flight = 1; }
            }
        }
        // ---- the free flight.  Curved rays: the transitions of LightPath::run_flight, one per trip of a wave-uniform loop
        if (CURVED) {
            int go = flight && (ev == EV_NONE || ev == EV_ARRIVED || ev == EV_EXITED);
            uint32_t pc = 0; bool pin = false;               // the cell of W.p
            if (go) pin = fluence_cell(G, W.p, pc);
            while (__ballot(go != 0)) {
                int mode = 0;                                // 1: one piece in hand (the chord stayed in its cell), 2: D walks the chord
                float h = 0.0f, pl = 0.0f; uint32_t c = 0;
                if (go) {
                    if (ev == EV_NONE) {
                        if (C.marched >= PT_STEP_BUDGET) ev = EV_GATE_FAIL;
                        else {
                            const f3 p0 = W.p; const int bs0 = W.backstep;
                            h = W.steps_left > 0 ? P.sc.stepsize : W.rem;
                            ev = W.advance(P, lp.rng, C);
                            uint32_t nc; const bool nin = fluence_cell(G, W.p, nc);
                            if (!bs0 && !W.backstep && h > 0.0f) {             // the step passed the inside test
                                inside += (double) h;
                                if (pin && nin && pc == nc) { mode = 1; c = pc; pl = h; }
                                else { float pre; if (D.begin(G, p0, W.p - p0, 1.0f, pre)) mode = 2; outside += (double) (pre * h); }
                            }
                            pc = nc; pin = nin;
                        }
                    } else if (ev == EV_ARRIVED) ev = W.on_arrived(P, lp.rng, C, sigma);
                    else ev = EV_FAIL;                       // EV_EXITED
                    go = ev == EV_NONE || ev == EV_ARRIVED || ev == EV_EXITED;
                }
                while (__ballot(mode != 0)) {
                    bool got = false;
                    if (mode == 1) { got = true; mode = 0; }
                    else if (mode == 2) {
                        float a, l, post_a, post;
                        if (!D.next(G, a, l, c, post_a, post)) { mode = 0; outside += (double) (post * h); }
                        pl = l * h; got = pl > 0.0f;
                    }
                    const bool flush = got && run_on && c != run_cell;
                    wave_deposit(G.sums, G.chk, CHK_SENSITIVITY, n_keys, flush, kbase + run_cell, w * run_l);
                    if (got) {
                        if (flush || !run_on) { run_cell = c; run_l = pl; run_on = 1; }
                        else run_l += pl;
                    }
                }
            }
        } else if (flight) ev = lp.run_flight(P, C, W, ev, sigma);
        float fL = 0.0f;                                     // straight: the length flown, [0, m.t] or [0, itsT]
        bool kdep = false; uint32_t kcell = 0;               // scatter: the collision's deposit
        if (flight) {
            if (ev == EV_REAL) {
                MRec m;
                if (lp.collide(P, C, W, sigma, m)) {
                    fL = m.t;
                    if (scatter) {
                        collisions++;
                        kdep = fluence_cell(G, m.p, kcell);
                        if (!kdep) collisions_out++;
                    }
                    lp.scatter(S, lp.arrive(W, m));
                }
            } else if (ev != EV_GATE_FAIL) { escaped = lp.T * lp.power; left = 1; fL = itsT; dexit = lp.exit_distance(W); }
        }
        // ---- the deposits: every lane of the wave makes every call of every trip (scatter is the launch's)
        if (scatter) wave_deposit(G.sums, G.chk, CHK_SENSITIVITY, n_keys, kdep, n_meas * (uint32_t) G.n_cells + kbase + kcell, w);
        if (CURVED) {
            wave_deposit(G.sums, G.chk, CHK_SENSITIVITY, n_keys, run_on != 0, kbase + run_cell, w * run_l);      // the flight ended: flush the run
            run_on = 0;
        } else {
            int pend = 0;
            if (fL > 0.0f && fL < MER_INF) {
                inside += (double) fL;
                float pre; pend = D.begin(G, fo, fd, fL, pre); outside += (double) pre;
            }
            while (__ballot(pend != 0)) {
                bool got = false; uint32_t c = 0; float l = 0.0f;
                if (pend) {
                    float a, post_a, post;
                    pend = D.next(G, a, l, c, post_a, post);
                    if (!pend) outside += (double) post;
                    got = l > 0.0f;
                }
                wave_deposit(G.sums, G.chk, CHK_SENSITIVITY, n_keys, got, kbase + c, w * l);
            }
        }
    }
    lp.weigh_exit(P, dexit, escaped);

    // the replayed exit against the record, bit for bit
    const bool agree = left && __float_as_uint(escaped.x) == __float_as_uint(w.x) && __float_as_uint(escaped.y) == __float_as_uint(w.y) &&
                       __float_as_uint(escaped.z) == __float_as_uint(w.z);
    const double tot[7] = {wave_sum_f64((double) w.x * outside), wave_sum_f64((double) w.y * outside), wave_sum_f64((double) w.z * outside),
                           wave_sum_f64((double) w.x * inside), wave_sum_f64((double) w.y * inside), wave_sum_f64((double) w.z * inside),
                           (double) wave_sum(have && !agree ? 1u : 0u)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            if (tot[q] != 0.0) atomicAdd(G.totals + 4 + q, tot[q]);
            if (tot[3 + q] != 0.0) atomicAdd(G.totals + 9 + q, tot[3 + q]);
        }
        if (tot[6] != 0.0) atomicAdd(G.totals + 12, tot[6]);
    }
    if (scatter) {
        const double co = (double) collisions_out;
        const double out[3] = {wave_sum_f64((double) w.x * co), wave_sum_f64((double) w.y * co), wave_sum_f64((double) w.z * co)};
        if ((threadIdx.x & 63) == 0) {
#pragma unroll
            for (int q = 0; q < 3; q++) if (out[q] != 0.0) atomicAdd(G.totals + 13 + q, out[q]);
        }
        wave_measure(G.totals + SENS_TOTALS, G.chk, n_meas, have && collisions != 0, kbase / (uint32_t) G.n_cells, 4,
                     (double) w.x * (double) collisions, (double) w.y * (double) collisions, (double) w.z * (double) collisions, 0.0);
    }
}

}  // namespace mer
