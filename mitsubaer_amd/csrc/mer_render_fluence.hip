// mer_render_fluence.hip -- the fluence grid recorded from light paths: instantiations of K_fluence (mer_fluence.hpp), its launch
// (launch_light_paths, mer_lightpath_host.hpp) and the mer_fluence_* entry points.  A grid is one device allocation: double[nz][ny][nx][3]
// sums, then the 8 totals; a time-resolved grid (mer_fluence_time_create) is double[frames][nz][ny][nx][3] sums, then 12 totals, and renders
// with the TIMED instantiations.  A track-length grid (mer_fluence_track_create) has the steady-state layout and renders with K_fluence_track
// (mer_render_fluence_track.hip).
#include "mer_lightpath_host.hpp"
#include "mer_fluence.hpp"

namespace mer {

template <bool TIMED> struct FluenceFamily {
    typedef void (*Kernel)(const Params, const FluenceGrid, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return fluence_kernel<CURVED, RIF, STEPPER, SIGMA, TIMED>; }
};
typedef FluenceFamily<false>::Kernel FluenceKernel;

// mer_render_fluence_track.hip: the same 14 combinations of K_fluence_track, for a handle of mer_fluence_track_create
FluenceKernel pick_fluence_track(const mer_scene_desc *sc);

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

static Fluence *find_fluence(mer_context *ctx, mer_fluence h, const char *who) { return find_sums(ctx, ctx->fluences, h, who, "fluence"); }
static int alloc_fluence(mer_context *ctx, Fluence &F, const char *who, mer_fluence *out) {
    return alloc_sums(ctx, ctx->fluences, F, std::string(who) + ": clearing the grid failed", out);
}

static int launch_fluence(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, const Fluence &F) {
    if (scene->integrator != MER_INTEGRATOR_PTRACER)
        return fail(ctx, "mer_render_fluence: the scene's integrator must be ptracer (the grid is recorded from light paths)");
    Params P;
    if (make_params(ctx, scene, P, false)) return 1;
    if (check_light_paths(ctx, P, shard)) return 1;
    if (F.track() && scene->sigma_mode != MER_SIGMA_GRID) {
        // the track-length weight is built for ANALOG distance sampling: every free flight drawn from one exponential exp(-rho s)
        const std::string at = "mer_render_fluence: a track-length grid needs analog distance sampling (one exponential per free flight): ";
        if (P.medium_sampling_weight != 1.0f) return fail(ctx, at + "medium_sampling_weight must be 1");
        if (scene->strategy == MER_STRATEGY_MAXIMUM) return fail(ctx, at + "strategy maximum samples the maximum of three exponentials");
        if (scene->strategy == MER_STRATEGY_BALANCE && !(P.sigT.x == P.sigT.y && P.sigT.y == P.sigT.z))
            return fail(ctx, at + "strategy balance with a channel-dependent sigma_t samples a mixture of exponentials");
    }
    FluenceGrid G;
    G.sums = F.dev; G.totals = F.totals(); G.chk = ctx->chk; G.n_cells = F.n_cells;
    G.frames = F.frames; G.t_min = F.t_min; G.t_bin = F.t_bin;
    for (int a = 0; a < 3; a++) { G.res[a] = F.desc.res[a]; G.bmin[a] = F.desc.bmin[a]; G.bmax[a] = F.desc.bmax[a]; }
    const FluenceKernel kernel = F.track() ? pick_fluence_track(scene) : F.timed() ? pick_light_kernel<FluenceFamily<true>>(scene) : pick_light_kernel<FluenceFamily<false>>(scene);
    return launch_light_paths(ctx, scene, P, shard, seed, nullptr, 0, kernel, G);
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
    return clear_sums(ctx, *F);
}

int mer_fluence_destroy(mer_context *ctx, mer_fluence h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Fluence *F = find_fluence(ctx, h, "mer_fluence_destroy");
    if (!F) return 1;
    return destroy_sums(ctx, ctx->fluences, h, *F);
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
    return read_sums(ctx, *F, sums, totals, 8);
}

int mer_fluence_time_read(mer_context *ctx, mer_fluence h, double *sums, double totals[12]) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Fluence *F = find_fluence(ctx, h, "mer_fluence_time_read");
    if (!F) return 1;
    if (!F->timed()) return fail(ctx, "mer_fluence_time_read: steady-state grid: use mer_fluence_read");
    if (!totals) return fail(ctx, "mer_fluence_time_read: invalid arguments");
    return read_sums(ctx, *F, sums, totals, 12);       // [11] is never written: 0
}

}
