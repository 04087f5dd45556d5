// mer_render_exitance.hip -- the exitance map recorded from light paths: instantiations of K_exitance (mer_exitance.hpp), its launch
// (launch_light_paths, mer_lightpath_host.hpp) and the mer_exitance_* entry points.  A map is one device allocation:
// double[frames][faces][res_v][res_u][3] sums, then the 16 totals.
#include "mer_lightpath_host.hpp"
#include "mer_exitance.hpp"

namespace mer {

struct ExitanceFamily {
    typedef void (*Kernel)(const Params, const ExitanceMap, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return exitance_kernel<CURVED, RIF, STEPPER, SIGMA>; }
};

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

static Exitance *find_exitance(mer_context *ctx, mer_exitance h, const char *who) { return find_sums(ctx, ctx->exitances, h, who, "exitance"); }

static int launch_exitance(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, const Exitance &E) {
    if (scene->integrator != MER_INTEGRATOR_PTRACER)
        return fail(ctx, "mer_render_exitance: the scene's integrator must be ptracer (the map is recorded from light paths)");
    Params P;
    if (make_params(ctx, scene, P, false)) return 1;
    if (scene->boundary != E.desc.boundary)
        return fail(ctx, "mer_render_exitance: the scene's boundary differs from the map's (a cube map has 6 faces, a sphere map 1)");
    if (check_light_paths(ctx, P, shard)) return 1;
    ExitanceMap M;
    M.sums = E.dev; M.totals = E.totals(); M.chk = ctx->chk;
    M.res_u = E.desc.res[0]; M.res_v = E.desc.res[1]; M.faces = E.faces(); M.frames = E.desc.frames;
    M.t_min = E.desc.t_min; M.t_bin = E.desc.t_bin; M.cos_min = E.desc.cos_min;
    return launch_light_paths(ctx, scene, P, shard, seed, nullptr, 0, pick_light_kernel<ExitanceFamily>(scene), M);
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
    return alloc_sums(ctx, ctx->exitances, E, "mer_exitance_create: clearing the map failed", out);
}

int mer_exitance_clear(mer_context *ctx, mer_exitance h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Exitance *E = find_exitance(ctx, h, "mer_exitance_clear");
    if (!E) return 1;
    return clear_sums(ctx, *E);
}

int mer_exitance_destroy(mer_context *ctx, mer_exitance h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Exitance *E = find_exitance(ctx, h, "mer_exitance_destroy");
    if (!E) return 1;
    return destroy_sums(ctx, ctx->exitances, h, *E);
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
    return read_sums(ctx, *E, sums, totals, 16);       // [15] is never written: 0
}

}
