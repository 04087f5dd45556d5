// mer_fluence.hpp -- the fluence inside the medium as a voxel grid, recorded from light paths (mer_render_fluence): a grid of the reference's
// `fluencemeter` probes (src/sensors/fluencemeter.cpp:40-41, driven by `ptracer`) instead of one probe per render.
//
// A light path is the walk of mer_lightpath.hpp, without the light tracer's sensor connection.  Every real collision the loop reaches is a
// collision-estimator sample of the fluence: w = T power (transmittance / pdfSuccess), taken before T is multiplied by the albedo, goes into
// the cell that holds the collision point (mer.h, mer_render_fluence, has the estimator in full).
//
// One lane runs one path, as in K_ptracer, but the event loop is WAVE-UNIFORM: it runs while any lane of the wave has a live path, and a lane
// whose path has ended idles through the body.  All 64 lanes therefore meet at the single deposit site at the end of the body, outside the
// lane-dependent free-flight loop, where wave_deposit merges the deposits of equal cells over the wave before it touches memory.
//
// TIMED (a handle of mer_fluence_time_create): the same walk, which also carries the light tracer's optical path length `plen`
// (float32: the exterior leg at index 1, then m.opticalLength or m.t * rif_const per free flight) and bins every deposit by it:
// frame = floorf((plen - t_min) / t_bin), key = frame * n_cells + cell.  The window is the handle's own; the film fields stay ignored.
//
// FD (a handle of mer_fluence_fd_create): the same walk and the same plen, and every deposit goes, as w (cos, sin)(k_j plen), into the
// 2 n_freq planes of the grid (wave_deposit_fd, mer_lightpath.hpp) at the same wave-converged site.  There is no window.
#pragma once
#include "mer_lightpath.hpp"

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
// A frequency-domain handle: sums = double[n_freq][2][nz][ny][nx][3], frames = 2 n_freq planes, totals = double[8], and behind the totals
// the wavenumbers, float64[MER_MAX_FREQUENCIES], in the recorder's own buffer.  No kernel argument is added for them: the plane loop
// indexes them with a scalar, eight doubles by value would be 16 kernel-argument SGPRs, and even a pointer and a count beside the grid --
// three SGPRs that the compiler loads at the kernel's entry and keeps across the event loop -- cost the straight gridded instance of
// K_exitance 36 bytes of scratch
__device__ __forceinline__ const double *fluence_wavenumbers(const FluenceGrid &G) { return G.totals + 8; }

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

// K_fluence.  The deposit's key is the cell; TIMED: frame * n_cells + cell, and the extent is the time-resolved grid's; FD: the cell in
// each of the 2 n_freq planes.  TIMED and FD exclude each other.
template <bool CURVED, int RIF, int STEPPER, int SIGMA, bool TIMED, bool FD = false>
__global__ void __launch_bounds__(PT_BLOCK) fluence_kernel(const Params P, const FluenceGrid G, uint64_t first, uint32_t count) {
    const mer_scene_desc &S = P.sc;
    LaneCounters C; C.clear();
    LightPath<CURVED, SIGMA> lp;
    f3 escaped(0, 0, 0);                                     // a path escapes once
    float dexit = -1.0f;                                     // ... after a flight of this length that reached the boundary (LightPath::weigh_exit)
    double dropped[3] = {0.0, 0.0, 0.0};
    uint32_t ended = 0;
    float plen = 0.0f;                                       // TIMED, FD: the optical path length, accumulated in float32 as K_ptracer does under a TRANSIENT film
    double late[3] = {0.0, 0.0, 0.0};                        // TIMED: the weight of deposits inside the box but outside the time window
    int x, y; float tIn;
    const int how = lp.decode(P, C, first, count, x, y) ? lp.emit(P, tIn) : LP_DEAD;
    if (how == LP_ENTERED) { if (TIMED || FD) plen += tIn; }
    else if (how == LP_MISSED) escaped = lp.power;

    Walk<CURVED, RIF, STEPPER, SIGMA> W;
    for (int event = 0; event < PT_MAX_EVENTS; ++event) {
        if (!__ballot(lp.alive != 0)) break;                 // wave-uniform: the wave leaves when its last path has ended
        bool dep = false; uint32_t cell = 0; f3 w(0, 0, 0);
        if (lp.alive) {
            lp.alive = 0;
            if (lp.can_fly()) {
                const float itsT = lp.boundary_distance(S);
                if (!(itsT >= 0)) escaped = lp.T * lp.power; // on the boundary, heading out
                else {
                    float sigma = 0.0f;
                    const int ev = lp.run_flight(P, C, W, lp.begin_flight(P, C, W, itsT), sigma);
                    if (ev == EV_REAL) {
                        MRec m;
                        if (!lp.collide(P, C, W, sigma, m)) ended++;
                        else {
                            // ---- the deposit: before the albedo
                            w = lp.T * lp.power * (m.transmittance / m.pdfSuccess);
                            dep = fluence_cell(G, m.p, cell);
                            if (!dep) { dropped[0] += (double) w.x; dropped[1] += (double) w.y; dropped[2] += (double) w.z; }
                            if (TIMED || FD) plen += CURVED ? m.opticalLength : m.t * S.rif_const;
                            if (TIMED) {
                                if (dep) {
                                    const float b = floorf((plen - G.t_min) / G.t_bin);                  // film_contribute's bin
                                    if (b >= 0.0f && b < (float) G.frames) cell += (uint32_t) b * (uint32_t) G.n_cells;      // the key, below 2^27
                                    else { dep = false; late[0] += (double) w.x; late[1] += (double) w.y; late[2] += (double) w.z; }
                                }
                            }
                            lp.scatter(S, lp.arrive(W, m));
                        }
                    } else if (ev == EV_GATE_FAIL) ended++;
                    else { escaped = lp.T * lp.power; dexit = lp.exit_distance(W); }       // the path left the convex shape
                }
            }
        }
        if constexpr (FD) wave_deposit_fd(G.sums, G.chk, CHK_FLUENCE, (uint32_t) G.n_cells, fluence_wavenumbers(G), G.frames >> 1, dep, cell, w, plen);
        else wave_deposit(G.sums, G.chk, CHK_FLUENCE, TIMED ? G.n_keys() : G.n_cells, dep, cell, w);
    }
    if (lp.alive) ended++;                                   // PT_MAX_EVENTS
    lp.weigh_exit(P, dexit, escaped);

    // totals and counters: one wave-aggregated flush each (every lane of the wave gets here)
    const double tot[8] = {(double) wave_sum(C.paths), wave_sum_f64((double) escaped.x), wave_sum_f64((double) escaped.y), wave_sum_f64((double) escaped.z),
                           wave_sum_f64(dropped[0]), wave_sum_f64(dropped[1]), wave_sum_f64(dropped[2]), (double) wave_sum(ended)};
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
    }
    flush_counters(P, C);
}

}  // namespace mer
