// mer_render_fluence.hip -- the fluence grid recorded from light paths: instantiations of K_fluence (mer_fluence.hpp), its host loop (the
// light tracer's: launches of PT_PATHS_PER_LAUNCH / PT_PATHS_PER_LAUNCH_CURVED paths on the context stream, returned synchronised) and the
// mer_fluence_* entry points.  A grid is one device allocation: double[nz][ny][nx][3] sums, then the 8 totals; a time-resolved grid
// (mer_fluence_time_create) is double[frames][nz][ny][nx][3] sums, then 12 totals, and renders with the TIMED instantiations.  A track-length
// grid (mer_fluence_track_create) has the steady-state layout and renders with K_fluence_track (mer_render_fluence_track.hip).
#include "mer_internal.hpp"
#include "mer_fluence.hpp"

namespace mer {

typedef void (*FluenceKernel)(const Params, const FluenceGrid, uint64_t, uint32_t);

// the 14 instantiations pick_ptracer (mer_render_ptracer.hip) selects from, once per kind of handle
template <bool CURVED, int RIF, int STEPPER, bool TIMED> static FluenceKernel pick_sigma(int sigma) {
    return sigma == MER_SIGMA_GRID ? fluence_kernel<CURVED, RIF, STEPPER, MER_SIGMA_GRID, TIMED> : fluence_kernel<CURVED, RIF, STEPPER, MER_SIGMA_HOMOGENEOUS, TIMED>;
}
template <int RIF, bool TIMED> static FluenceKernel pick_curved(int stepper, int sigma) {
    if (stepper == MER_STEP_VERLET) return pick_sigma<true, RIF, MER_STEP_VERLET, TIMED>(sigma);
    if (stepper == MER_STEP_RK4) return pick_sigma<true, RIF, MER_STEP_RK4, TIMED>(sigma);
    return nullptr;
}
template <bool TIMED> static FluenceKernel pick_fluence(const mer_scene_desc *sc) {
    const int sigma = sc->sigma_mode == MER_SIGMA_GRID ? MER_SIGMA_GRID : MER_SIGMA_HOMOGENEOUS;
    switch (sc->rif_mode) {
    case MER_RIF_CONST: return pick_sigma<false, MER_RIF_TRILINEAR, MER_STEP_VERLET, TIMED>(sigma);
    case MER_RIF_TRILINEAR: return pick_curved<MER_RIF_TRILINEAR, TIMED>(sc->stepper, sigma);
    case MER_RIF_BSPLINE3: return pick_curved<MER_RIF_BSPLINE3, TIMED>(sc->stepper, sigma);
    case MER_RIF_ACOUSTIC: return pick_curved<RIFK_ACOUSTIC, TIMED>(sc->stepper, sigma);
    }
    return nullptr;
}

// mer_render_fluence_track.hip: the same 14 combinations of K_fluence_track, for a handle of mer_fluence_track_create
FluenceKernel pick_fluence_track(const mer_scene_desc *sc);

static int check_fluence_desc(mer_context *ctx, const mer_fluence_desc *d, const std::string &at = "mer_fluence_create: ") {
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

// the box checks of mer_fluence_create, then the window's
static int check_fluence_time_desc(mer_context *ctx, const mer_fluence_time_desc *d) {
    const std::string at = "mer_fluence_time_create: ";
    mer_fluence_desc box;
    for (int a = 0; a < 3; a++) { box.res[a] = d->res[a]; box.bmin[a] = d->bmin[a]; box.bmax[a] = d->bmax[a]; }
    if (check_fluence_desc(ctx, &box, at)) return 1;
    if (d->frames < 1 || d->frames > 4096) return fail(ctx, at + "frames must lie in 1 ... 4096");
    if (!std::isfinite(d->t_min)) return fail(ctx, at + "t_min must be finite");
    if (!std::isfinite(d->t_bin) || !(d->t_bin > 0)) return fail(ctx, at + "t_bin must be finite and greater than 0");
    if (d->reserved != 0) return fail(ctx, at + "reserved must be 0");
    const uint64_t cells = (uint64_t) d->res[0] * (uint64_t) d->res[1] * (uint64_t) d->res[2];
    if (cells * (uint64_t) d->frames > ((uint64_t) 1 << 27)) return fail(ctx, at + "more than 2^27 cells x frames");
    return 0;
}

// the zeroed device buffer of a checked grid and its handle
static int alloc_fluence(mer_context *ctx, Fluence &F, const char *who, mer_fluence *out) {
    HIP_CHECK(ctx, hipMalloc((void **) &F.dev, F.bytes()));
    if (hipMemsetAsync(F.dev, 0, F.bytes(), ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void) hipFree(F.dev);
        return fail(ctx, std::string(who) + ": clearing the grid failed");
    }
    const int h = ctx->next_handle++;
    ctx->fluences[h] = F;
    *out = h;
    return 0;
}

static Fluence *find_fluence(mer_context *ctx, mer_fluence h, const char *who) {
    auto it = ctx->fluences.find(h);
    if (it == ctx->fluences.end()) { ctx->error = std::string(who) + ": unknown fluence handle"; return nullptr; }
    return &it->second;
}

static int launch_fluence(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, const Fluence &F) {
    if (scene->integrator != MER_INTEGRATOR_PTRACER)
        return fail(ctx, "mer_render_fluence: the scene's integrator must be ptracer (the grid is recorded from light paths)");
    Params P;
    if (make_params(ctx, scene, P, false)) return 1;
    if (!shard || shard->spp_count < 0 || shard->spp_stride <= 0 || shard->tile_count <= 0 || shard->tile_rank < 0 ||
        shard->tile_rank >= shard->tile_count || shard->spp_begin < 0)
        return fail(ctx, "invalid shard");
    if (P.n_point <= 0) return fail(ctx, "ptracer: the scene has no emitter (list entries of kind point, spot or collimated)");
    if (F.track() && scene->sigma_mode != MER_SIGMA_GRID) {
        // the track-length weight is built for ANALOG distance sampling: every free flight drawn from one exponential exp(-rho s)
        const std::string at = "mer_render_fluence: a track-length grid needs analog distance sampling (one exponential per free flight): ";
        if (P.medium_sampling_weight != 1.0f) return fail(ctx, at + "medium_sampling_weight must be 1");
        if (scene->strategy == MER_STRATEGY_MAXIMUM) return fail(ctx, at + "strategy maximum samples the maximum of three exponentials");
        if (scene->strategy == MER_STRATEGY_BALANCE && !(P.sigT.x == P.sigT.y && P.sigT.y == P.sigT.z))
            return fail(ctx, at + "strategy balance with a channel-dependent sigma_t samples a mixture of exponentials");
    }
    const FluenceKernel kernel = F.track() ? pick_fluence_track(scene) : F.timed() ? pick_fluence<true>(scene) : pick_fluence<false>(scene);
    if (!kernel) return fail(ctx, "unsupported rif_mode / stepper combination");
    // the work ids of the shard, as launch_ptracer lays them out (decode_work)
    P.seed = seed;
    P.spp_begin = shard->spp_begin; P.spp_count = shard->spp_count; P.spp_stride = shard->spp_stride;
    P.tile_rank = shard->tile_rank; P.tile_count = shard->tile_count;
    P.tiles_x = (scene->width + MER_TILE - 1) / MER_TILE; P.tiles_y = (scene->height + MER_TILE - 1) / MER_TILE;
    P.tile_skew = tile_skew_for(P.tiles_x, shard->tile_count, (int) ctx->opt.tile_deal);
    const int ntiles = P.tiles_x * P.tiles_y;
    P.ntiles_mine = (ntiles - shard->tile_rank + shard->tile_count - 1) / shard->tile_count;
    P.total_work = (uint64_t) P.ntiles_mine * MER_TILE * MER_TILE * (uint64_t) shard->spp_count;
    P.film = nullptr; P.path_out = nullptr; P.n_film = 0; P.n_path_out = 0;          // no film: the sensor fields only enumerate the paths
    FluenceGrid G;
    G.sums = F.dev; G.totals = F.totals(); G.chk = ctx->chk; G.n_cells = F.n_cells;
    G.frames = F.frames; G.t_min = F.t_min; G.t_bin = F.t_bin;
    for (int a = 0; a < 3; a++) { G.res[a] = F.desc.res[a]; G.bmin[a] = F.desc.bmin[a]; G.bmax[a] = F.desc.bmax[a]; }
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (P.total_work == 0) return 0;
    HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    const uint64_t chunk = scene->rif_mode == MER_RIF_CONST ? PT_PATHS_PER_LAUNCH : PT_PATHS_PER_LAUNCH_CURVED;
    for (uint64_t first = 0; first < P.total_work; first += chunk) {
        const uint32_t count = (uint32_t) std::min<uint64_t>(chunk, P.total_work - first);
        hipLaunchKernelGGL(kernel, dim3((count + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, ctx->stream, P, G, first, count);
        HIP_CHECK(ctx, hipGetLastError());
    }
    HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));
    ctx->last_event_ms = 0; ctx->last_march_ms = 0; ctx->last_passes = 0; ctx->last_pipes = 1;
    return 0;
}

}  // namespace mer

using namespace mer;

extern "C" {

int mer_fluence_create(mer_context *ctx, const mer_fluence_desc *desc, mer_fluence *out) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    if (!desc || !out) return fail(ctx, "mer_fluence_create: invalid arguments");
    *out = 0;
    if (check_fluence_desc(ctx, desc)) return 1;
    Fluence F;
    F.desc = *desc;
    F.n_cells = (uint64_t) desc->res[0] * (uint64_t) desc->res[1] * (uint64_t) desc->res[2];
    return alloc_fluence(ctx, F, "mer_fluence_create", out);
}

int mer_fluence_track_create(mer_context *ctx, const mer_fluence_desc *desc, mer_fluence *out) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    if (!desc || !out) return fail(ctx, "mer_fluence_track_create: invalid arguments");
    *out = 0;
    if (check_fluence_desc(ctx, desc, "mer_fluence_track_create: ")) return 1;
    Fluence F;
    F.desc = *desc;
    F.n_cells = (uint64_t) desc->res[0] * (uint64_t) desc->res[1] * (uint64_t) desc->res[2];
    F.kind = 1;
    return alloc_fluence(ctx, F, "mer_fluence_track_create", out);
}

int mer_fluence_time_create(mer_context *ctx, const mer_fluence_time_desc *desc, mer_fluence *out) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    if (!desc || !out) return fail(ctx, "mer_fluence_time_create: invalid arguments");
    *out = 0;
    if (check_fluence_time_desc(ctx, desc)) return 1;
    Fluence F;
    for (int a = 0; a < 3; a++) { F.desc.res[a] = desc->res[a]; F.desc.bmin[a] = desc->bmin[a]; F.desc.bmax[a] = desc->bmax[a]; }
    F.n_cells = (uint64_t) desc->res[0] * (uint64_t) desc->res[1] * (uint64_t) desc->res[2];
    F.frames = desc->frames; F.t_min = desc->t_min; F.t_bin = desc->t_bin;
    return alloc_fluence(ctx, F, "mer_fluence_time_create", out);
}

int mer_fluence_clear(mer_context *ctx, mer_fluence h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Fluence *F = find_fluence(ctx, h, "mer_fluence_clear");
    if (!F) return 1;
    HIP_CHECK(ctx, hipMemsetAsync(F->dev, 0, F->bytes(), ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int mer_fluence_destroy(mer_context *ctx, mer_fluence h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Fluence *F = find_fluence(ctx, h, "mer_fluence_destroy");
    if (!F) return 1;
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    (void) hipFree(F->dev);
    ctx->fluences.erase(h);
    return 0;
}

int mer_render_fluence(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_fluence h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    if (!scene) return fail(ctx, "mer_render_fluence: no scene");
    const Fluence *F = find_fluence(ctx, h, "mer_render_fluence");
    if (!F) return 1;
    return launch_fluence(ctx, scene, shard, seed, *F);
}

int mer_fluence_read(mer_context *ctx, mer_fluence h, double *sums, double totals[8]) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Fluence *F = find_fluence(ctx, h, "mer_fluence_read");
    if (!F) return 1;
    if (F->timed()) return fail(ctx, "mer_fluence_read: time-resolved grid: use mer_fluence_time_read");
    if (!totals) return fail(ctx, "mer_fluence_read: invalid arguments");
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (sums) HIP_CHECK(ctx, hipMemcpy(sums, F->dev, F->n_cells * 3 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(ctx, hipMemcpy(totals, F->totals(), 8 * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

int mer_fluence_time_read(mer_context *ctx, mer_fluence h, double *sums, double totals[12]) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Fluence *F = find_fluence(ctx, h, "mer_fluence_time_read");
    if (!F) return 1;
    if (!F->timed()) return fail(ctx, "mer_fluence_time_read: steady-state grid: use mer_fluence_read");
    if (!totals) return fail(ctx, "mer_fluence_time_read: invalid arguments");
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (sums) HIP_CHECK(ctx, hipMemcpy(sums, F->dev, F->n_keys() * 3 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(ctx, hipMemcpy(totals, F->totals(), 12 * sizeof(double), hipMemcpyDeviceToHost));       // [11] is never written: 0
    return 0;
}

}
