// mer_lightpath_host.hpp -- the host side every light-path kernel family shares (mer_render_ptracer.hip, mer_render_fluence.hip,
// mer_render_fluence_track.hip, mer_render_exitance.hip, mer_render_sensitivity.hip): the choice among a family's 14 instantiations, the launch
// loop over the work ids of a shard, and the device buffer behind a mer_fluence / mer_exitance / mer_sensitivity handle.
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

// ---- One render from light paths.  P is the caller's make_params(ctx, scene, P, false): each entry point makes it among refusals of its
// own, in its own order (and the track-length grid has more to refuse between the checks and the launch), so the launcher comes in two steps.
// The shard and the emitters:
static inline int check_light_paths(mer_context *ctx, const Params &P, const mer_shard *shard) {
    if (!shard || shard->spp_count < 0 || shard->spp_stride <= 0 || shard->tile_count <= 0 || shard->tile_rank < 0 ||
        shard->tile_rank >= shard->tile_count || shard->spp_begin < 0)
        return fail(ctx, "invalid shard");
    if (P.n_point <= 0) return fail(ctx, "ptracer: the scene has no emitter (list entries of kind point, spot or collimated)");
    return 0;
}
// The light paths of a shard are the (pixel, sample index) pairs K_gen would enumerate: the work ids are laid out as launch_render lays them
// out (decode_work) and launched PT_PATHS_PER_LAUNCH (curved rays: PT_PATHS_PER_LAUNCH_CURVED) at a time on the context stream as
// kernel(P, extra ..., first, count).  Returns synchronised, as the wavefront loop does.  film = nullptr: the sensor fields only enumerate the paths.
// The loop itself: per_chunk(first, count) launches what one chunk of work ids needs and returns nonzero (with the context's message set) to stop.
template <class PerChunk>
static int for_light_path_chunks(mer_context *ctx, const mer_scene_desc *scene, Params &P, const mer_shard *shard, uint64_t seed, float *film_dev,
                                 uint64_t n_film, PerChunk per_chunk) {
    P.seed = seed;
    P.spp_begin = shard->spp_begin; P.spp_count = shard->spp_count; P.spp_stride = shard->spp_stride;
    P.tile_rank = shard->tile_rank; P.tile_count = shard->tile_count;
    P.tiles_x = (scene->width + MER_TILE - 1) / MER_TILE; P.tiles_y = (scene->height + MER_TILE - 1) / MER_TILE;
    P.tile_skew = tile_skew_for(P.tiles_x, shard->tile_count, (int) ctx->opt.tile_deal);
    const int ntiles = P.tiles_x * P.tiles_y;
    P.ntiles_mine = (ntiles - shard->tile_rank + shard->tile_count - 1) / shard->tile_count;
    P.total_work = (uint64_t) P.ntiles_mine * MER_TILE * MER_TILE * (uint64_t) shard->spp_count;
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
static int launch_light_paths(mer_context *ctx, const mer_scene_desc *scene, Params &P, const mer_shard *shard, uint64_t seed, float *film_dev,
                              uint64_t n_film, Kernel kernel, const Extra &... extra) {
    if (!kernel) return fail(ctx, "unsupported rif_mode / stepper combination");
    return for_light_path_chunks(ctx, scene, P, shard, seed, film_dev, n_film, [&](uint64_t first, uint32_t count) {
        hipLaunchKernelGGL(kernel, dim3((count + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, ctx->stream, P, extra..., first, count);
        HIP_CHECK(ctx, hipGetLastError());
        return 0;
    });
}

// ---- The box of a voxel grid over the medium (fluence grids, sensitivity grids): the checks of mer_fluence_create under the caller's prefix
static inline int check_fluence_desc(mer_context *ctx, const mer_fluence_desc *d, const std::string &at = "mer_fluence_create: ") {
    uint64_t cells = 1;
    for (int a = 0; a < 3; a++) {
        if (d->res[a] < 1 || d->res[a] > 1024) return fail(ctx, at + "res must lie in 1 ... 1024 on every axis");
        if (!std::isfinite(d->bmin[a]) || !std::isfinite(d->bmax[a])) return fail(ctx, at + "bmin / bmax must be finite");
        if (!(d->bmin[a] < d->bmax[a])) return fail(ctx, at + "bmin must be below bmax on every axis");
        cells *= (uint64_t) d->res[a];
    }
    if (cells > ((uint64_t) 1 << 27)) return fail(ctx, at + "more than 2^27 cells");
    return 0;
}

// ---- The device buffer behind a handle H (Fluence, Exitance: mer_internal.hpp): n_keys() * 3 sums, then the totals, bytes() in all.
// `what` names the kind of handle in messages ("fluence" / "exitance"); the two kinds keep a map each, so a handle of one is unknown to the other.
template <class H> static H *find_sums(mer_context *ctx, std::map<int, H> &handles, int h, const char *who, const char *what) {
    auto it = handles.find(h);
    if (it == handles.end()) { ctx->error = std::string(who) + ": unknown " + what + " handle"; return nullptr; }
    return &it->second;
}
// the zeroed buffer of a checked description and its handle
template <class H> static int alloc_sums(mer_context *ctx, std::map<int, H> &handles, H &v, const std::string &clearing_failed, int *out) {
    HIP_CHECK(ctx, hipMalloc((void **) &v.dev, v.bytes()));
    if (hipMemsetAsync(v.dev, 0, v.bytes(), ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void) hipFree(v.dev);
        return fail(ctx, clearing_failed);
    }
    const int h = ctx->next_handle++;
    handles[h] = v;
    *out = h;
    return 0;
}
template <class H> static int clear_sums(mer_context *ctx, const H &v) {
    HIP_CHECK(ctx, hipMemsetAsync(v.dev, 0, v.bytes(), ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
template <class H> static int destroy_sums(mer_context *ctx, std::map<int, H> &handles, int h, const H &v) {
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    (void) hipFree(v.dev);
    handles.erase(h);
    return 0;
}
// sums (optional) and the first n_totals totals
template <class H> static int read_sums(mer_context *ctx, const H &v, double *sums, double *totals, int n_totals) {
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (sums) HIP_CHECK(ctx, hipMemcpy(sums, v.dev, v.n_keys() * 3 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(ctx, hipMemcpy(totals, v.totals(), (size_t) n_totals * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}  // namespace mer
