// mer_fluence_track.hpp -- the track-length estimator of the fluence grid (a handle of mer_fluence_track_create): the light path of
// mer_lightpath.hpp, as K_fluence (mer_fluence.hpp) walks it, but instead of one deposit at the real collision every free flight deposits along the piece of path it flew inside the shape, cut at the faces of the grid's
// cells.  Cell c, crossed between the flight parameters a and b (arc length from the flight's start), receives per channel
//     w_c = T_c power_c  integral_a^b tau_c(s) / S(s) ds,         S(s) = the probability that the sampled distance exceeds s,
// which is unbiased for any distance sampling (E[integral_0^min(t, L) f / S] = integral_0^L f) and is built here for S = exp(-rho s):
// rho = sigma(x) for delta tracking in a gridded sigma_t (w = T power (b - a)), rho = the sampling density of a homogeneous medium whose every
// flight is drawn from one exponential (mer_render_fluence refuses the others).  With Delta_c = sigma_t,c - rho and l = b - a:
//     w_c = T_c power_c exp(-Delta_c a) (-expm1(-Delta_c l)) / Delta_c,       exactly T_c power_c l when Delta_c == 0.
// The deposit draws no sampler number, so counters, escaped weight and ended paths equal K_fluence's for the same scene, shard and seed.
// Pieces outside the box add their w to the `dropped` total (weight x length).
//
// One lane runs one path and the event loop is wave-uniform, as in K_fluence.  Straight rays: the resolved flight [0, m.t] or [0, itsT] is
// walked cell by cell (TrackDDA) in a wave-uniform loop, one piece per lane per trip, and every trip ends in wave_deposit, which
// merges the pieces of equal cells over the wave -- a collimated beam keeps all 64 lanes in one column in lockstep.  Curved rays: the stepping
// loop itself is wave-uniform; a step that passed the inside test deposits along its chord W.p(before) -> W.p(after) at the arc length W.dist
// (the step that left the shape and the step back after it deposit nothing, so the last piece before the boundary, shorter than one step, is
// lost as it is for the walk).  A lane keeps a run (cell, summed w) in registers while its chords stay in one cell and flushes it when the
// cell changes or the flight ends: atomics scale with the cells a path crosses, not with its steps.
#pragma once
#include "mer_fluence.hpp"          // FluenceGrid, fluence_cell

namespace mer {

// w of one piece [a, a + l) of a flight: Tp = T * power at the flight's start, delta = sigma_t - rho per channel (HOMOG only)
template <bool HOMOG>
__device__ __forceinline__ f3 track_weight(f3 Tp, f3 delta, float a, float l) {
    if (!HOMOG) return Tp * l;
    return f3(delta.x == 0.0f ? Tp.x * l : Tp.x * expf(-delta.x * a) * (-expm1f(-delta.x * l)) / delta.x,
              delta.y == 0.0f ? Tp.y * l : Tp.y * expf(-delta.y * a) * (-expm1f(-delta.y * l)) / delta.y,
              delta.z == 0.0f ? Tp.z * l : Tp.z * expf(-delta.z * a) * (-expm1f(-delta.z * l)) / delta.z);
}

// The cells of the grid that x(t) = o + d t crosses for t in [0, tend], in order: begin() clips against the box, next() hands out one piece
// per call.  A component of d that is exactly 0 never divides: its inverse is stored as 0 and means "no plane of this axis is crossed".
// The indices stay inside the grid for every piece handed out; the walk ends when it steps off the grid, reaches the box's far side or has
// handed out res_x + res_y + res_z pieces (a line crosses fewer cells).
struct TrackDDA {
    f3 o, inv;
    float tc, t1, tend;
    int32_t ix, iy, iz, trips;

    static __device__ __forceinline__ float plane(const FluenceGrid &G, int a, int32_t k) {
        return G.bmin[a] + (G.bmax[a] - G.bmin[a]) * ((float) k / (float) G.res[a]);
    }
    static __device__ __forceinline__ int32_t index(const FluenceGrid &G, int a, float x) {
        const float f = floorf((x - G.bmin[a]) / (G.bmax[a] - G.bmin[a]) * (float) G.res[a]);           // fluence_cell's expression
        return (int32_t) fminf(fmaxf(f, 0.0f), (float) (G.res[a] - 1));                                 // a NaN ends as 0
    }
    // false: no part of [0, tend] lies in the box.  pre = the length in front of the box (all of it when false).
    __device__ __forceinline__ bool begin(const FluenceGrid &G, f3 o_, f3 d, float tend_, float &pre) {
        o = o_; tend = tend_; trips = G.res[0] + G.res[1] + G.res[2];
        inv = f3(d.x != 0.0f ? 1.0f / d.x : 0.0f, d.y != 0.0f ? 1.0f / d.y : 0.0f, d.z != 0.0f ? 1.0f / d.z : 0.0f);
        float t0 = 0.0f, te = tend_; bool hit = true;
        const float oo[3] = {o.x, o.y, o.z}, ii[3] = {inv.x, inv.y, inv.z};
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (ii[a] != 0.0f) {
                const float ta = (G.bmin[a] - oo[a]) * ii[a], tb = (G.bmax[a] - oo[a]) * ii[a];
                t0 = fmaxf(t0, fminf(ta, tb)); te = fminf(te, fmaxf(ta, tb));
            } else if (!(oo[a] >= G.bmin[a] && oo[a] < G.bmax[a])) hit = false;                          // half-open, as the cells are
        }
        pre = tend_;
        if (!(hit && t0 < te)) return false;
        pre = t0; tc = t0; t1 = te;
        const f3 pe = o + d * t0;
        ix = index(G, 0, pe.x); iy = index(G, 1, pe.y); iz = index(G, 2, pe.z);
        return true;
    }
    // The next piece: [a, a + l) in `cell` (l may be 0 at a face).  false: it was the last one, and [post_a, post_a + post) is what is left
    // of [0, tend] behind the box.
    __device__ __forceinline__ bool next(const FluenceGrid &G, float &a, float &l, uint32_t &cell, float &post_a, float &post) {
        const float tx = inv.x != 0.0f ? (plane(G, 0, ix + (inv.x > 0.0f ? 1 : 0)) - o.x) * inv.x : MER_INF;
        const float ty = inv.y != 0.0f ? (plane(G, 1, iy + (inv.y > 0.0f ? 1 : 0)) - o.y) * inv.y : MER_INF;
        const float tz = inv.z != 0.0f ? (plane(G, 2, iz + (inv.z > 0.0f ? 1 : 0)) - o.z) * inv.z : MER_INF;
        float tn = fminf(fminf(tx, ty), tz);
        const bool far_side = !(tn < t1);
        if (far_side) tn = t1;
        a = tc; l = fmaxf(tn - tc, 0.0f);
        cell = ((uint32_t) iz * (uint32_t) G.res[1] + (uint32_t) iy) * (uint32_t) G.res[0] + (uint32_t) ix;
        tc = fmaxf(tc, tn);
        bool more = !far_side && --trips > 0;
        if (more) {
            if (tx <= ty && tx <= tz) { ix += inv.x > 0.0f ? 1 : -1; more = ix >= 0 && ix < G.res[0]; }
            else if (ty <= tz) { iy += inv.y > 0.0f ? 1 : -1; more = iy >= 0 && iy < G.res[1]; }
            else { iz += inv.z > 0.0f ? 1 : -1; more = iz >= 0 && iz < G.res[2]; }
        }
        post_a = tc; post = more ? 0.0f : fmaxf(tend - tc, 0.0f);
        return more;
    }
};

// K_fluence_track.  Every deposit is a wave_deposit over the steady-state grid's cells.
template <bool CURVED, int RIF, int STEPPER, int SIGMA>
__global__ void __launch_bounds__(PT_BLOCK) fluence_track_kernel(const Params P, const FluenceGrid G, uint64_t first, uint32_t count) {
    constexpr bool HOMOG = SIGMA == MER_SIGMA_HOMOGENEOUS;
    const mer_scene_desc &S = P.sc;
    LaneCounters C; C.clear();
    LightPath<CURVED, SIGMA> lp;
    f3 escaped(0, 0, 0);
    float dexit = -1.0f;                                     // the length of the flight that reached the boundary (LightPath::weigh_exit)
    double dropped[3] = {0.0, 0.0, 0.0};                     // weight x length of the pieces outside the box
    uint32_t ended = 0;
    int x, y; float tIn;
    if (lp.decode(P, C, first, count, x, y) && lp.emit(P, tIn) == LP_MISSED) escaped = lp.power;

    Walk<CURVED, RIF, STEPPER, SIGMA> W;
    TrackDDA D;
    uint32_t run_cell = 0; f3 run_w(0, 0, 0); int run_on = 0;            // CURVED: the lane's run of chords in one cell
    for (int event = 0; event < PT_MAX_EVENTS; ++event) {
        if (!__ballot(lp.alive != 0)) break;
        int ev = EV_FAIL, flight = 0;
        float itsT = 0.0f, sigma = 0.0f;
        const f3 fo = lp.ps, fd = lp.dcur, fT = lp.T * lp.power;          // the flight's start, direction and T power
        f3 delta(0, 0, 0);
        auto drop = [&](float a, float l) {
            if (l > 0.0f) {
                const f3 w = track_weight<HOMOG>(fT, delta, a, l);
                dropped[0] += (double) w.x; dropped[1] += (double) w.y; dropped[2] += (double) w.z;
            }
        };
        if (lp.alive) {
            lp.alive = 0;
            if (lp.can_fly()) {
                itsT = lp.boundary_distance(S);
                if (!(itsT >= 0)) escaped = fT;
                else {
                    ev = lp.begin_flight(P, C, W, itsT);
                    flight = 1;
                    if (HOMOG) delta = f3(P.sigT.x - W.sdens, P.sigT.y - W.sdens, P.sigT.z - W.sdens);       // rho = the density the flight was drawn with
                }
            }
        }
        // ---- the free flight.  Curved rays: the transitions of LightPath::run_flight, one per trip of a wave-uniform loop
        if (CURVED) {
            int go = flight && (ev == EV_NONE || ev == EV_ARRIVED || ev == EV_EXITED);
            uint32_t pc = 0; bool pin = false;               // the cell of W.p
            if (go) pin = fluence_cell(G, W.p, pc);
            while (__ballot(go != 0)) {
                int mode = 0;                                // 1: one piece in hand (the chord stayed in its cell), 2: D walks the chord
                float a0 = 0.0f, h = 0.0f, pa = 0.0f, pl = 0.0f; uint32_t c = 0;
                if (go) {
                    if (ev == EV_NONE) {
                        if (C.marched >= PT_STEP_BUDGET) ev = EV_GATE_FAIL;
                        else {
                            const f3 p0 = W.p; const int bs0 = W.backstep;
                            a0 = W.dist; h = W.steps_left > 0 ? P.sc.stepsize : W.rem;
                            ev = W.advance(P, lp.rng, C);
                            uint32_t nc; const bool nin = fluence_cell(G, W.p, nc);
                            if (!bs0 && !W.backstep && h > 0.0f) {             // the step passed the inside test
                                if (pin && nin && pc == nc) { mode = 1; c = pc; pa = a0; pl = h; }
                                else { float pre; if (D.begin(G, p0, W.p - p0, 1.0f, pre)) mode = 2; drop(a0, pre * h); }
                            }
                            pc = nc; pin = nin;
                        }
                    } else if (ev == EV_ARRIVED) ev = W.on_arrived(P, lp.rng, C, sigma);
                    else ev = EV_FAIL;                       // EV_EXITED
                    go = ev == EV_NONE || ev == EV_ARRIVED || ev == EV_EXITED;
                }
                while (__ballot(mode != 0)) {
                    bool have = false; f3 w(0, 0, 0);
                    if (mode == 1) { have = true; mode = 0; }
                    else if (mode == 2) {
                        float a, l, post_a, post;
                        if (!D.next(G, a, l, c, post_a, post)) { mode = 0; drop(a0 + post_a * h, post * h); }
                        pa = a0 + a * h; pl = l * h; have = pl > 0.0f;
                    }
                    if (have) w = track_weight<HOMOG>(fT, delta, pa, pl);
                    const bool flush = have && run_on && c != run_cell;
                    wave_deposit(G.sums, G.chk, CHK_FLUENCE, G.n_cells, flush, run_cell, run_w);
                    if (have) {
                        if (flush || !run_on) { run_cell = c; run_w = w; run_on = 1; }
                        else run_w = run_w + w;
                    }
                }
            }
        } else if (flight) ev = lp.run_flight(P, C, W, ev, sigma);
        float fL = 0.0f;                                     // straight: the length flown, [0, m.t] or [0, itsT]
        if (flight) {
            if (ev == EV_REAL) {
                MRec m;
                if (!lp.collide(P, C, W, sigma, m)) ended++;
                else {
                    fL = m.t;
                    lp.scatter(S, lp.arrive(W, m));
                }
            } else if (ev == EV_GATE_FAIL) ended++;
            else { escaped = fT; fL = itsT; dexit = lp.exit_distance(W); }
        }
        // ---- the deposits
        if (CURVED) {
            wave_deposit(G.sums, G.chk, CHK_FLUENCE, G.n_cells, run_on != 0, run_cell, run_w);      // the flight ended: flush the run
            run_on = 0;
        } else {
            int pend = 0;
            if (fL > 0.0f && fL < MER_INF) { float pre; pend = D.begin(G, fo, fd, fL, pre); drop(0.0f, pre); }
            while (__ballot(pend != 0)) {
                bool have = false; uint32_t c = 0; f3 w(0, 0, 0);
                if (pend) {
                    float a, l, post_a, post;
                    pend = D.next(G, a, l, c, post_a, post);
                    if (!pend) drop(post_a, post);
                    have = l > 0.0f;
                    if (have) w = track_weight<HOMOG>(fT, delta, a, l);
                }
                wave_deposit(G.sums, G.chk, CHK_FLUENCE, G.n_cells, have, c, w);
            }
        }
    }
    if (lp.alive) ended++;                                   // PT_MAX_EVENTS
    lp.weigh_exit(P, dexit, escaped);

    const double tot[8] = {(double) wave_sum(C.paths), wave_sum_f64((double) escaped.x), wave_sum_f64((double) escaped.y), wave_sum_f64((double) escaped.z),
                           wave_sum_f64(dropped[0]), wave_sum_f64(dropped[1]), wave_sum_f64(dropped[2]), (double) wave_sum(ended)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 8; q++) if (tot[q] != 0.0) atomicAdd(G.totals + q, tot[q]);
    }
    flush_counters(P, C);
}

}  // namespace mer
