// mer_exitance.hpp -- where and when light paths leave the medium: a map of the escaped weight over the boundary of the medium shape
// (mer_render_exitance), a grid of the reference's `irradiancemeter` probes (src/sensors/irradiancemeter.cpp, driven by `ptracer`) instead of
// one probe per render.
//
// A light path is the walk of mer_lightpath.hpp.  Recording an exit draws no sampler number, fetches no RIF value and advances no counter, so
// counters, paths, escaped weight and ended paths equal K_fluence's.  At each place where K_fluence sets `escaped` the lane notes the exit
// point x, the outward direction d, the same weight w (LightPath::weigh_exit for a flight that reached the boundary) and the optical path length l
// (mer.h, mer_render_exitance, has the estimator in full).
//
// With the null boundary and a convex shape a path leaves at most once, so a lane keeps its one (key, w) in registers and the wave deposits
// ONCE, after the event loop, with all 64 lanes converged (wave_deposit).  The event loop itself needs no wave-uniform trip count for the
// deposit; it keeps K_fluence's form.
//
// FD (a handle of mer_exitance_fd_create): the same exit, deposited as w (cos, sin)(k_j l) into the 2 n_freq planes of the map
// (wave_deposit_fd, mer_lightpath.hpp) at the same site.  The cone applies; there is no window.
#pragma once
#include "mer_lightpath.hpp"

namespace mer {

// the map of one mer_exitance handle on the device: sums = double[frames][faces][res_v][res_u][3], totals = double[16] (mer.h)
struct ExitanceMap {
    double *sums, *totals;
    unsigned long long *chk;
    int32_t res_u, res_v, faces, frames;
    float t_min, t_bin, cos_min;
    __host__ __device__ uint64_t n_keys() const { return (uint64_t) frames * (uint64_t) faces * (uint64_t) res_v * (uint64_t) res_u; }
};

// A frequency-domain handle: sums = double[n_freq][2][faces][res_v][res_u][3], frames = 2 n_freq planes, t_bin = 0, and the wavenumbers
// lie behind the 16 totals, as FluenceGrid has it (mer_fluence.hpp)
__device__ __forceinline__ const double *exitance_wavenumbers(const ExitanceMap &M) { return M.totals + 16; }

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

// K_exitance
template <bool CURVED, int RIF, int STEPPER, int SIGMA, bool FD = false>
__global__ void __launch_bounds__(PT_BLOCK) exitance_kernel(const Params P, const ExitanceMap M, uint64_t first, uint32_t count) {
    const mer_scene_desc &S = P.sc;
    LaneCounters C; C.clear();
    LightPath<CURVED, SIGMA> lp;
    f3 escaped(0, 0, 0);                                     // a path escapes once
    int miss = 0;                                            // ... through the boundary at xe heading de after the path length plen (dexit >= 0), or without meeting the shape
    f3 xe(0, 0, 0), de(0, 0, 1);
    float dexit = -1.0f;                                     // >= 0: the path left through the boundary, after a flight of this length (LightPath::weigh_exit; 0: from the boundary itself)
    uint32_t ended = 0;
    float plen = 0.0f;                                       // the optical path length, accumulated in float32 as K_fluence does for a time-resolved grid
    int x, y; float tIn;
    const int how = lp.decode(P, C, first, count, x, y) ? lp.emit(P, tIn) : LP_DEAD;
    if (how == LP_ENTERED) plen += tIn;
    else if (how == LP_MISSED) { escaped = lp.power; miss = 1; }      // the emitted ray misses the shape: no exit point

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
                        // the path left the convex shape.  The walk's own state is read as it stands: finish_free_flight(..., false, ...)
                        // would fetch the RIF on a curved ray and count it
                        escaped = lp.T * lp.power; dexit = lp.exit_distance(W); lp.weigh_exit(P, dexit, escaped);
                        if (CURVED) {
                            // W.pos() is the last point inside; the shape is met again along the momentum (the re-hit of the dielectric
                            // boundary, mer_wavefront.hpp).  The piece x0 -> x, shorter than one stepsize, adds nothing to the path length.
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

    // ---- the one deposit of the path: cone (tested first), window, cell.  Every lane of the wave gets here.
    double rejected[3] = {0.0, 0.0, 0.0}, late[3] = {0.0, 0.0, 0.0}, missed[3] = {0.0, 0.0, 0.0};
    bool dep = false; uint32_t key = 0;
    if (miss) { missed[0] = (double) escaped.x; missed[1] = (double) escaped.y; missed[2] = (double) escaped.z; }
    if (dexit >= 0.0f) {
        dep = true;
        if (M.cos_min > 0.0f && dot(de, shape_normal(S, xe)) < M.cos_min) {
            dep = false; rejected[0] = (double) escaped.x; rejected[1] = (double) escaped.y; rejected[2] = (double) escaped.z;
        } else if (!FD && M.t_bin > 0.0f) {
            const float b = floorf((plen - M.t_min) / M.t_bin);
            if (b >= 0.0f && b < (float) M.frames) key = (uint32_t) b * (uint32_t) (M.faces * M.res_v * M.res_u);      // the key stays below 2^27
            else { dep = false; late[0] = (double) escaped.x; late[1] = (double) escaped.y; late[2] = (double) escaped.z; }
        }
        if (dep) key += exitance_cell(S, M, xe);
    }
    if constexpr (FD) wave_deposit_fd(M.sums, M.chk, CHK_EXITANCE, (uint32_t) (M.faces * M.res_v * M.res_u), exitance_wavenumbers(M), M.frames >> 1, dep, key, escaped, plen);
    else wave_deposit(M.sums, M.chk, CHK_EXITANCE, M.n_keys(), dep, key, escaped);

    // totals and counters: one wave-aggregated flush each
    const double tot[15] = {(double) wave_sum(C.paths), wave_sum_f64((double) escaped.x), wave_sum_f64((double) escaped.y), wave_sum_f64((double) escaped.z),
                            wave_sum_f64(missed[0]), wave_sum_f64(missed[1]), wave_sum_f64(missed[2]), (double) wave_sum(ended),
                            wave_sum_f64(late[0]), wave_sum_f64(late[1]), wave_sum_f64(late[2]),
                            wave_sum_f64(rejected[0]), wave_sum_f64(rejected[1]), wave_sum_f64(rejected[2]), (double) wave_sum(dep ? 1u : 0u)};
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < 15; q++) if (tot[q] != 0.0) atomicAdd(M.totals + q, tot[q]);
    }
    flush_counters(P, C);
}

}  // namespace mer
