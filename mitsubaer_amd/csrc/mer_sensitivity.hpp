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
#pragma once
#include "mer_exitance.hpp"         // ExitanceMap, exitance_cell
#include "mer_fluence_track.hpp"    // FluenceGrid, fluence_cell, TrackDDA

namespace mer {

// the detected-path list of a context: SoA, so that the lanes of a wave write (and K_replay's read) adjacent words.  id = the work id less
// the launch's `first`.  cap = the paths of one launch chunk: the list cannot overflow.  One pointer, DETECT_HEAD words whose first is the
// count, then the four arrays of cap words; the kernels form the arrays' addresses themselves: with a pointer per array, and a whole
// ExitanceMap in the detector, four K_detect instances had 36 bytes of scratch (SGPR pressure from the kernel arguments).
#define DETECT_HEAD 64
struct DetectList {
    uint32_t *count;
    uint32_t cap;
    unsigned long long *chk;
    __device__ __forceinline__ uint32_t *id() const { return count + DETECT_HEAD; }
    __device__ __forceinline__ float *w(int c) const { return (float *) (count + DETECT_HEAD + (size_t) (c + 1) * cap); }
};

// the detector of a mer_sensitivity handle: the raster, the window, the cone and the gate
struct Detector {
    int32_t res_u, res_v, face, iu0, iu1, iv0, iv1;
    float cos_min, t_min, t_bin;
};

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

// K_detect.  totals (mer.h): [0] paths, [1..3] the detected weight, [7] ended, [8] the detected paths.
template <bool CURVED, int RIF, int STEPPER, int SIGMA>
__global__ void __launch_bounds__(PT_BLOCK) detect_kernel(const Params P, const Detector D, const DetectList L, double *totals, uint64_t first, uint32_t count) {
    const mer_scene_desc &S = P.sc;
    LaneCounters C; C.clear();
    ExitRecord R;
    exit_walk<CURVED, RIF, STEPPER, SIGMA>(P, C, first, count, R);

    // ---- the detector: cone (tested first), gate, window.  Every lane of the wave gets here.
    bool det = false;
    if (R.dexit >= 0.0f) {
        det = !(D.cos_min > 0.0f && dot(R.de, shape_normal(S, R.xe)) < D.cos_min);
        if (det && D.t_bin > 0.0f) det = floorf((R.plen - D.t_min) / D.t_bin) == 0.0f;
        if (det) {
            ExitanceMap M; M.res_u = D.res_u; M.res_v = D.res_v;         // all that exitance_cell reads of a map
            const uint32_t cell = exitance_cell(S, M, R.xe), row = cell / (uint32_t) D.res_u;
            const int32_t iu = (int32_t) (cell - row * (uint32_t) D.res_u), iv = (int32_t) (row % (uint32_t) D.res_v), face = (int32_t) (row / (uint32_t) D.res_v);
            det = face == D.face && iu >= D.iu0 && iu < D.iu1 && iv >= D.iv0 && iv < D.iv1;
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
        }
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
template <bool CURVED, int RIF, int STEPPER, int SIGMA>
__global__ void __launch_bounds__(PT_BLOCK) replay_kernel(const Params P, const FluenceGrid G, const DetectList L, uint64_t first, uint32_t n) {
    const mer_scene_desc &S = P.sc;
    LaneCounters C; C.clear();
    LightPath<CURVED, SIGMA> lp;
    const uint32_t r = blockIdx.x * PT_BLOCK + threadIdx.x;
    const bool have = r < n;
    uint32_t j = 0; f3 w(0, 0, 0);
    if (have) {
        const uint64_t at = MER_CHK(L.chk, CHK_DETECT_LIST, r, L.cap);
        j = L.id()[at]; w = f3(L.w(0)[at], L.w(1)[at], L.w(2)[at]);
    }
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
                    wave_deposit(G.sums, G.chk, CHK_SENSITIVITY, G.n_cells, flush, run_cell, w * run_l);
                    if (got) {
                        if (flush || !run_on) { run_cell = c; run_l = pl; run_on = 1; }
                        else run_l += pl;
                    }
                }
            }
        } else if (flight) ev = lp.run_flight(P, C, W, ev, sigma);
        float fL = 0.0f;                                     // straight: the length flown, [0, m.t] or [0, itsT]
        if (flight) {
            if (ev == EV_REAL) {
                MRec m;
                if (lp.collide(P, C, W, sigma, m)) {
                    fL = m.t;
                    lp.scatter(S, lp.arrive(W, m));
                }
            } else if (ev != EV_GATE_FAIL) { escaped = lp.T * lp.power; left = 1; fL = itsT; dexit = lp.exit_distance(W); }
        }
        // ---- the deposits
        if (CURVED) {
            wave_deposit(G.sums, G.chk, CHK_SENSITIVITY, G.n_cells, run_on != 0, run_cell, w * run_l);      // the flight ended: flush the run
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
                wave_deposit(G.sums, G.chk, CHK_SENSITIVITY, G.n_cells, got, c, w * l);
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
}

}  // namespace mer
