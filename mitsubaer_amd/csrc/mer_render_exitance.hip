// mer_render_exitance.hip -- the exitance map recorded from light paths: instantiations of K_exitance (mer_exitance.hpp) in the 14 combinations
// pick_fluence (mer_render_fluence.hip) selects from, its host loop (the light tracer's: launches of PT_PATHS_PER_LAUNCH /
// PT_PATHS_PER_LAUNCH_CURVED paths on the context stream, returned synchronised) and the mer_exitance_* entry points.  A map is one device
// allocation: double[frames][faces][res_v][res_u][3] sums, then the 16 totals.
#include "mer_internal.hpp"
#include "mer_exitance.hpp"

namespace mer {

typedef void (*ExitanceKernel)(const Params, const ExitanceMap, uint64_t, uint32_t);

template <bool CURVED, int RIF, int STEPPER> static ExitanceKernel pick_sigma(int sigma) {
    return sigma == MER_SIGMA_GRID ? exitance_kernel<CURVED, RIF, STEPPER, MER_SIGMA_GRID> : exitance_kernel<CURVED, RIF, STEPPER, MER_SIGMA_HOMOGENEOUS>;
}
template <int RIF> static ExitanceKernel pick_curved(int stepper, int sigma) {
    if (stepper == MER_STEP_VERLET) return pick_sigma<true, RIF, MER_STEP_VERLET>(sigma);
    if (stepper == MER_STEP_RK4) return pick_sigma<true, RIF, MER_STEP_RK4>(sigma);
    return nullptr;
}
static ExitanceKernel pick_exitance(const mer_scene_desc *sc) {
    const int sigma = sc->sigma_mode == MER_SIGMA_GRID ? MER_SIGMA_GRID : MER_SIGMA_HOMOGENEOUS;
    switch (sc->rif_mode) {
    case MER_RIF_CONST: return pick_sigma<false, MER_RIF_TRILINEAR, MER_STEP_VERLET>(sigma);
    case MER_RIF_TRILINEAR: return pick_curved<MER_RIF_TRILINEAR>(sc->stepper, sigma);
    case MER_RIF_BSPLINE3: return pick_curved<MER_RIF_BSPLINE3>(sc->stepper, sigma);
    case MER_RIF_ACOUSTIC: return pick_curved<RIFK_ACOUSTIC>(sc->stepper, sigma);
    }
    return nullptr;
}

static int check_exitance_desc(mer_context *ctx, const mer_exitance_desc *d) {
    const std::string at = "mer_exitance_create: ";
    if (d->boundary != MER_BOUNDARY_AABB && d->boundary != MER_BOUNDARY_SPHERE) return fail(ctx, at + "boundary must be the cube (MER_BOUNDARY_AABB) or the sphere (MER_BOUNDARY_SPHERE)");
    for (int a = 0; a < 2; a++)
        if (d->res[a] < 1 || d->res[a] > 4096) return fail(ctx, at + "res must lie in 1 ... 4096 on both axes");
    if (d->frames < 1 || d->frames > 4096) return fail(ctx, at + "frames must lie in 1 ... 4096");
    if (!std::isfinite(d->t_bin) || d->t_bin < 0) return fail(ctx, at + "t_bin must be finite and at least 0");
    if (d->t_bin == 0 && d->frames != 1) return fail(ctx, at + "a steady map (t_bin == 0) has one frame");
    if (!std::isfinite(d->t_min)) return fail(ctx, at + "t_min must be finite");
    if (!(d->cos_min >= 0 && d->cos_min < 1)) return fail(ctx, at + "cos_min must lie in 0 <= cos_min < 1");
    if (d->reserved != 0) return fail(ctx, at + "reserved must be 0");
    const uint64_t faces = d->boundary == MER_BOUNDARY_SPHERE ? 1 : 6;
    if ((uint64_t) d->frames * faces * (uint64_t) d->res[0] * (uint64_t) d->res[1] > ((uint64_t) 1 << 27)) return fail(ctx, at + "more than 2^27 cells x faces x frames");
    return 0;
}

static Exitance *find_exitance(mer_context *ctx, mer_exitance h, const char *who) {
    auto it = ctx->exitances.find(h);
    if (it == ctx->exitances.end()) { ctx->error = std::string(who) + ": unknown exitance handle"; return nullptr; }
    return &it->second;
}

static int launch_exitance(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, const Exitance &E) {
    if (scene->integrator != MER_INTEGRATOR_PTRACER)
        return fail(ctx, "mer_render_exitance: the scene's integrator must be ptracer (the map is recorded from light paths)");
    Params P;
    if (make_params(ctx, scene, P, false)) return 1;
    if (scene->boundary != E.desc.boundary)
        return fail(ctx, "mer_render_exitance: the scene's boundary differs from the map's (a cube map has 6 faces, a sphere map 1)");
    if (!shard || shard->spp_count < 0 || shard->spp_stride <= 0 || shard->tile_count <= 0 || shard->tile_rank < 0 ||
        shard->tile_rank >= shard->tile_count || shard->spp_begin < 0)
        return fail(ctx, "invalid shard");
    if (P.n_point <= 0) return fail(ctx, "ptracer: the scene has no emitter (list entries of kind point, spot or collimated)");
    const ExitanceKernel kernel = pick_exitance(scene);
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
    ExitanceMap M;
    M.sums = E.dev; M.totals = E.totals(); M.chk = ctx->chk;
    M.res_u = E.desc.res[0]; M.res_v = E.desc.res[1]; M.faces = E.faces(); M.frames = E.desc.frames;
    M.t_min = E.desc.t_min; M.t_bin = E.desc.t_bin; M.cos_min = E.desc.cos_min;
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    if (P.total_work == 0) return 0;
    HIP_CHECK(ctx, hipEventRecord(ctx->ev0, ctx->stream));
    const uint64_t chunk = scene->rif_mode == MER_RIF_CONST ? PT_PATHS_PER_LAUNCH : PT_PATHS_PER_LAUNCH_CURVED;
    for (uint64_t first = 0; first < P.total_work; first += chunk) {
        const uint32_t count = (uint32_t) std::min<uint64_t>(chunk, P.total_work - first);
        hipLaunchKernelGGL(kernel, dim3((count + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, ctx->stream, P, M, first, count);
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

int mer_exitance_create(mer_context *ctx, const mer_exitance_desc *desc, mer_exitance *out) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    if (!desc || !out) return fail(ctx, "mer_exitance_create: invalid arguments");
    *out = 0;
    if (check_exitance_desc(ctx, desc)) return 1;
    Exitance E;
    E.desc = *desc;
    HIP_CHECK(ctx, hipMalloc((void **) &E.dev, E.bytes()));
    if (hipMemsetAsync(E.dev, 0, E.bytes(), ctx->stream) != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess) {
        (void) hipFree(E.dev);
        return fail(ctx, "mer_exitance_create: clearing the map failed");
    }
    const int h = ctx->next_handle++;
    ctx->exitances[h] = E;
    *out = h;
    return 0;
}

int mer_exitance_clear(mer_context *ctx, mer_exitance h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Exitance *E = find_exitance(ctx, h, "mer_exitance_clear");
    if (!E) return 1;
    HIP_CHECK(ctx, hipMemsetAsync(E->dev, 0, E->bytes(), ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int mer_exitance_destroy(mer_context *ctx, mer_exitance h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Exitance *E = find_exitance(ctx, h, "mer_exitance_destroy");
    if (!E) return 1;
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    (void) hipFree(E->dev);
    ctx->exitances.erase(h);
    return 0;
}

int mer_render_exitance(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_exitance h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    if (!scene) return fail(ctx, "mer_render_exitance: no scene");
    const Exitance *E = find_exitance(ctx, h, "mer_render_exitance");
    if (!E) return 1;
    return launch_exitance(ctx, scene, shard, seed, *E);
}

int mer_exitance_read(mer_context *ctx, mer_exitance h, double *sums, double totals[16]) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Exitance *E = find_exitance(ctx, h, "mer_exitance_read");
    if (!E) return 1;
    if (!totals) return fail(ctx, "mer_exitance_read: invalid arguments");
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    if (sums) HIP_CHECK(ctx, hipMemcpy(sums, E->dev, E->n_keys() * 3 * sizeof(double), hipMemcpyDeviceToHost));
    HIP_CHECK(ctx, hipMemcpy(totals, E->totals(), 16 * sizeof(double), hipMemcpyDeviceToHost));       // [15] is never written: 0
    return 0;
}

}
