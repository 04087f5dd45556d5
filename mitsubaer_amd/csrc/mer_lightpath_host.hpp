// mer_lightpath_host.hpp -- the host side every light-path kernel family shares (mer_render_ptracer.hip, mer_render_fluence.hip,
// mer_render_fluence_track.hip, mer_render_exitance.hip, mer_render_sensitivity.hip): the choice among a family's 14 instantiations, the launch
// loop over the work ids of a shard, and the Recorder behind a mer_fluence / mer_exitance / mer_sensitivity handle: its description's checks,
// its lookup by family, its device buffer and the shared opening of its launch.
#pragma once
#include "mer_internal.hpp"
#include "mer_lightpath.hpp"

namespace mer {

// ---- the 14 (CURVED, RIF, STEPPER, SIGMA) instantiations of a kernel family F: F::Kernel is the launchable pointer type and
// F::get<CURVED, RIF, STEPPER, SIGMA>() the instance.  A dense trilinear RIF is read with global loads whatever its size (the buffer-load
// fetch kind is a wavefront-kernel optimisation).  nullptr: a combination no family has.
template <class F, bool CURVED, int RIF, int STEPPER> static typename F::Kernel pick_sigma(int sigma) {
    return sigma == MER_SIGMA_GRID ? F::template get<CURVED, RIF, STEPPER, MER_SIGMA_GRID>() : F::template get<CURVED, RIF, STEPPER, MER_SIGMA_HOMOGENEOUS>();
}
template <class F, int RIF> static typename F::Kernel pick_curved(int stepper, int sigma) {
    if (stepper == MER_STEP_VERLET) return pick_sigma<F, true, RIF, MER_STEP_VERLET>(sigma);
    if (stepper == MER_STEP_RK4) return pick_sigma<F, true, RIF, MER_STEP_RK4>(sigma);
    return nullptr;
}
template <class F> static typename F::Kernel pick_light_kernel(const mer_scene_desc *sc) {
    const int sigma = sc->sigma_mode == MER_SIGMA_GRID ? MER_SIGMA_GRID : MER_SIGMA_HOMOGENEOUS;
    switch (sc->rif_mode) {
    case MER_RIF_CONST: return pick_sigma<F, false, MER_RIF_TRILINEAR, MER_STEP_VERLET>(sigma);
    case MER_RIF_TRILINEAR: return pick_curved<F, MER_RIF_TRILINEAR>(sc->stepper, sigma);
    case MER_RIF_BSPLINE3: return pick_curved<F, MER_RIF_BSPLINE3>(sc->stepper, sigma);
    case MER_RIF_ACOUSTIC: return pick_curved<F, RIFK_ACOUSTIC>(sc->stepper, sigma);
    }
    return nullptr;
}

// ---- One render from light paths.  The launcher comes in two steps: open_light_paths makes P = make_params(ctx, scene, P, false) among the
// refusals every recorder's launch shares, in their one order, and the launch follows once the caller has refused what is its own (the
// track-length grid's analog requirement) and filled its kernel arguments.  The light tracer itself (launch_ptracer) has other refusals around
// the same check of the shard (set_work, which also lays the shard's work ids out in P) and the emitters:
static inline int check_light_paths(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, Params &P) {
    if (set_work(ctx, scene, shard, P)) return 1;
    if (P.n_point <= 0) return fail(ctx, "ptracer: the scene has no emitter (list entries of kind point, spot or collimated)");
    return 0;
}
// not_ptracer / other_boundary: the entry point's own sentences; other_boundary = nullptr for a recorder without a boundary (the fluence grids)
static inline int open_light_paths(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, const Recorder &R, Params &P,
                                   const char *not_ptracer, const char *other_boundary) {
    if (scene->integrator != MER_INTEGRATOR_PTRACER) return fail(ctx, not_ptracer);
    if (make_params(ctx, scene, P, false)) return 1;
    if (other_boundary && scene->boundary != R.det.boundary) return fail(ctx, other_boundary);
    return check_light_paths(ctx, scene, shard, P);
}
// The light paths of a shard are the (pixel, sample index) pairs K_gen would enumerate: the work ids are laid out as launch_render lays them
// out (set_work, by check_light_paths above) and launched PT_PATHS_PER_LAUNCH (curved rays: PT_PATHS_PER_LAUNCH_CURVED) at a time on the context stream as
// kernel(P, extra ..., first, count).  Returns synchronised, as the wavefront loop does.  film = nullptr: the sensor fields only enumerate the paths.
// The loop itself: per_chunk(first, count) launches what one chunk of work ids needs and returns nonzero (with the context's message set) to stop.
template <class PerChunk>
static int for_light_path_chunks(mer_context *ctx, const mer_scene_desc *scene, Params &P, uint64_t seed, float *film_dev,
                                 uint64_t n_film, PerChunk per_chunk) {
    P.seed = seed;
    P.film = film_dev; P.path_out = nullptr; P.n_film = n_film; P.n_path_out = 0;
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (P.total_work == 0) return 0;
    HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    const uint64_t chunk = scene->rif_mode == MER_RIF_CONST ? PT_PATHS_PER_LAUNCH : PT_PATHS_PER_LAUNCH_CURVED;
    for (uint64_t first = 0; first < P.total_work; first += chunk) {
        const uint32_t count = (uint32_t) std::min<uint64_t>(chunk, P.total_work - first);
        if (per_chunk(first, count)) return 1;
    }
    HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));
    ctx->last_event_ms = 0; ctx->last_march_ms = 0; ctx->last_passes = 0; ctx->last_pipes = 1;
    return 0;
}
// one kernel per chunk, as kernel(P, extra ..., first, count)
template <class Kernel, class... Extra>
static int launch_light_paths(mer_context *ctx, const mer_scene_desc *scene, Params &P, uint64_t seed, float *film_dev,
                              uint64_t n_film, Kernel kernel, const Extra &... extra) {
    if (!kernel) return fail(ctx, "unsupported rif_mode / stepper combination");
    return for_light_path_chunks(ctx, scene, P, seed, film_dev, n_film, [&](uint64_t first, uint32_t count) {
        hipLaunchKernelGGL(kernel, dim3((count + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, ctx->stream, P, extra..., first, count);
        HIP_CHECK(ctx, hipGetLastError());
        return 0;
    });
}

// ---- The checks of a description, under the entry point's prefix.  The box of a voxel grid over the medium (fluence, sensitivity):
static inline int check_box(mer_context *ctx, const std::string &at, const int32_t res[3], const float bmin[3], const float bmax[3]) {
    uint64_t cells = 1;
    for (int a = 0; a < 3; a++) {
        if (res[a] < 1 || res[a] > 1024) return fail(ctx, at + "res must lie in 1 ... 1024 on every axis");
        if (!std::isfinite(bmin[a]) || !std::isfinite(bmax[a])) return fail(ctx, at + "bmin / bmax must be finite");
        if (!(bmin[a] < bmax[a])) return fail(ctx, at + "bmin must be below bmax on every axis");
        cells *= (uint64_t) res[a];
    }
    if (cells > ((uint64_t) 1 << 27)) return fail(ctx, at + "more than 2^27 cells");
    return 0;
}
// The raster on the boundary, its gate and its cone (exitance maps; the detector of a sensitivity grid, which has one frame).  res_what: "res" / "detector res"
static inline int check_raster(mer_context *ctx, const std::string &at, const char *res_what, const mer_detector_desc &t, int32_t frames) {
    if (t.boundary != MER_BOUNDARY_AABB && t.boundary != MER_BOUNDARY_SPHERE) return fail(ctx, at + "boundary must be the cube (MER_BOUNDARY_AABB) or the sphere (MER_BOUNDARY_SPHERE)");
    for (int a = 0; a < 2; a++)
        if (t.res[a] < 1 || t.res[a] > 4096) return fail(ctx, at + res_what + " must lie in 1 ... 4096 on both axes");
    if (frames < 1 || frames > 4096) return fail(ctx, at + "frames must lie in 1 ... 4096");
    if (!std::isfinite(t.t_bin) || t.t_bin < 0) return fail(ctx, at + "t_bin must be finite and at least 0");
    if (t.t_bin == 0 && frames != 1) return fail(ctx, at + "a steady map (t_bin == 0) has one frame");
    if (!std::isfinite(t.t_min)) return fail(ctx, at + "t_min must be finite");
    if (!(t.cos_min >= 0 && t.cos_min < 1)) return fail(ctx, at + "cos_min must lie in 0 <= cos_min < 1");
    if (t.reserved != 0) return fail(ctx, at + "reserved must be 0");
    return 0;
}

// The wavenumbers of a frequency-domain recorder (mer_fluence_fd_create, mer_exitance_fd_create) and the reserved words beside them
static inline int check_frequencies(mer_context *ctx, const std::string &at, int32_t n_freq, const double wavenumber[MER_MAX_FREQUENCIES], const int32_t *reserved, int n_reserved) {
    if (n_freq < 1 || n_freq > MER_MAX_FREQUENCIES) return fail(ctx, at + "n_freq must lie in 1 ... 8");
    for (int j = 0; j < n_freq; j++)
        if (!std::isfinite(wavenumber[j]) || wavenumber[j] < 0) return fail(ctx, at + "a wavenumber must be finite and at least 0");
    for (int j = n_freq; j < MER_MAX_FREQUENCIES; j++)
        if (!(wavenumber[j] == 0)) return fail(ctx, at + "the entries of wavenumber past n_freq must be 0");
    for (int q = 0; q < n_reserved; q++)
        if (reserved[q] != 0) return fail(ctx, at + "reserved must be 0");
    return 0;
}
// ... into the recorder; alloc_sums puts them behind the totals on the device
static inline void set_frequencies(Recorder &v, int32_t n_freq, const double wavenumber[MER_MAX_FREQUENCIES]) {
    v.kind = REC_FD; v.n_freq = n_freq;
    for (int j = 0; j < MER_MAX_FREQUENCIES; j++) v.wavenumber[j] = wavenumber[j];
}

// ---- The Recorder behind a handle (mer_internal.hpp).  Every entry point opens with one of these two: false / nullptr means return 1 (the
// message is set unless ctx is null).  create_args: the arguments of a *_create.
static inline bool create_args(mer_context *ctx, const void *desc, int *out, const char *who) {
    if (!ctx) return false;
    (void) hipSetDevice(ctx->device);
    if (!desc || !out) { ctx->error = std::string(who) + ": invalid arguments"; return false; }
    *out = 0;
    return true;
}
// find_recorder: the handle, which must be of the entry point's family -- one of another is as unknown as a number never issued.
// has_scene: the render entry points pass scene != nullptr
static inline Recorder *find_recorder(mer_context *ctx, int h, int family, const char *who, bool has_scene = true) {
    static const char *const names[3] = {"fluence", "exitance", "sensitivity"};
    if (!ctx) return nullptr;
    (void) hipSetDevice(ctx->device);
    if (!has_scene) { ctx->error = std::string(who) + ": no scene"; return nullptr; }
    auto it = ctx->recorders.find(h);
    if (it == ctx->recorders.end() || it->second.family != family) { ctx->error = std::string(who) + ": unknown " + names[family] + " handle"; return nullptr; }
    return &it->second;
}
// the zeroed buffer of a checked description (family, kind, n_keys and n_totals set) and its handle
static inline int alloc_sums(mer_context *ctx, Recorder &v, const std::string &clearing_failed, int *out) {
    if (v.dev.alloc(ctx, v.bytes())) return 1;
    if (hipMemsetAsync(v.dev.p, 0, v.bytes(), ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess)
        return fail(ctx, clearing_failed);
    if (v.fd()) HIP_CHECK(ctx, hipMemcpy(v.wavenumbers(), v.wavenumber, sizeof(v.wavenumber), hipMemcpyHostToDevice));
    const int h = ctx->next_handle++;
    ctx->recorders[h] = std::move(v);
    *out = h;
    return 0;
}
static inline int clear_sums(mer_context *ctx, const Recorder *v) {
    if (!v) return 1;
    HIP_CHECK(ctx, hipMemsetAsync(v->dev.p, 0, v->cleared_bytes(), ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
static inline int destroy_sums(mer_context *ctx, int h, const Recorder *v) {
    if (!v) return 1;
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    ctx->recorders.erase(h);
    return 0;
}
// sums (optional) and the totals, n_totals of them
static inline int read_sums(mer_context *ctx, const Recorder &v, double *sums, double *totals, const char *who) {
    if (!totals) return fail(ctx, std::string(who) + ": invalid arguments");
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (sums) HIP_CHECK(ctx, hipMemcpy(sums, v.sums(), v.n_keys * 3 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(ctx, hipMemcpy(totals, v.totals(), (size_t) v.n_totals * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}
// the voxel grid K_fluence, K_fluence_track and K_replay deposit into: the recorder's box, and the time bins of a timed fluence grid or the planes of a frequency-domain one
// (Grid = FluenceGrid, mer_fluence.hpp, which only the translation units of those kernels include)
template <class Grid> static Grid fluence_grid(const mer_context *ctx, const Recorder &R) {
    Grid G;
    G.sums = R.sums(); G.totals = R.totals(); G.chk = ctx->chk; G.n_cells = R.n_cells();
    G.frames = R.timed() ? R.frames : R.fd() ? 2 * R.n_freq : 0; G.t_min = R.timed() ? R.det.t_min : 0; G.t_bin = R.timed() ? R.det.t_bin : 0;
    for (int a = 0; a < 3; a++) { G.res[a] = R.box.res[a]; G.bmin[a] = R.box.bmin[a]; G.bmax[a] = R.box.bmax[a]; }
    return G;
}

}  // namespace mer
