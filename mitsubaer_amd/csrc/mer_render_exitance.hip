// mer_render_exitance.hip -- the exitance map recorded from light paths: instantiations of K_exitance (mer_exitance.hpp), its launch and the
// mer_exitance_* entry points, over the Recorder of family REC_EXITANCE and what mer_lightpath_host.hpp shares.  A frequency-domain map
// (mer_exitance_fd_create) renders with the FD instantiations (mer_render_exitance_fd.hip).
#include "mer_lightpath_host.hpp"
#include "mer_exitance.hpp"

namespace mer {

struct ExitanceFamily {
    typedef void (*Kernel)(const Params, const ExitanceMap, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return exitance_kernel<CURVED, RIF, STEPPER, SIGMA>; }
};

// mer_render_exitance_fd.hip: the same 14 combinations of the frequency-domain kind of K_exitance, for a handle of mer_exitance_fd_create
ExitanceFamily::Kernel pick_exitance_fd(const mer_scene_desc *sc);

static int launch_exitance(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, const Recorder &E) {
    Params P;
    if (open_light_paths(ctx, scene, shard, E, P, "mer_render_exitance: the scene's integrator must be ptracer (the map is recorded from light paths)",
                         "mer_render_exitance: the scene's boundary differs from the map's (a cube map has 6 faces, a sphere map 1)")) return 1;
    ExitanceMap M;
    M.sums = E.sums(); M.totals = E.totals(); M.chk = ctx->chk;
    M.res_u = E.det.res[0]; M.res_v = E.det.res[1]; M.faces = E.faces(); M.frames = E.frames;
    M.t_min = E.det.t_min; M.t_bin = E.det.t_bin; M.cos_min = E.det.cos_min;
    if (E.fd()) M.frames = 2 * E.n_freq;                     // the planes, in the place of the frames
    return launch_light_paths(ctx, scene, P, seed, nullptr, 0, E.fd() ? pick_exitance_fd(scene) : pick_light_kernel<ExitanceFamily>(scene), M);
}

}  // namespace mer

using namespace mer;

extern "C" {

int mer_exitance_create(mer_context *ctx, const mer_exitance_desc *d, mer_exitance *out) {
    if (!create_args(ctx, d, out, "mer_exitance_create")) return 1;
    Recorder E;
    E.family = REC_EXITANCE; E.n_totals = 16; E.frames = d->frames;
    E.det.boundary = d->boundary; E.det.res[0] = d->res[0]; E.det.res[1] = d->res[1];
    E.det.t_min = d->t_min; E.det.t_bin = d->t_bin; E.det.cos_min = d->cos_min; E.det.reserved = d->reserved;
    const std::string at = "mer_exitance_create: ";
    if (check_raster(ctx, at, "res", E.det, E.frames)) return 1;
    E.n_keys = (uint64_t) d->frames * (uint64_t) E.faces() * (uint64_t) d->res[1] * (uint64_t) d->res[0];
    if (E.n_keys > ((uint64_t) 1 << 27)) return fail(ctx, at + "more than 2^27 cells x faces x frames");
    return alloc_sums(ctx, E, "mer_exitance_create: clearing the map failed", out);
}

int mer_exitance_fd_create(mer_context *ctx, const mer_exitance_fd_desc *d, mer_exitance *out) {
    if (!create_args(ctx, d, out, "mer_exitance_fd_create")) return 1;
    Recorder E;
    E.family = REC_EXITANCE; E.n_totals = 16; E.frames = 1;
    E.det.boundary = d->boundary; E.det.res[0] = d->res[0]; E.det.res[1] = d->res[1]; E.det.cos_min = d->cos_min;
    const std::string at = "mer_exitance_fd_create: ";
    if (check_raster(ctx, at, "res", E.det, E.frames) || check_frequencies(ctx, at, d->n_freq, d->wavenumber, &d->reserved, 1)) return 1;
    E.n_keys = (uint64_t) (2 * d->n_freq) * (uint64_t) E.faces() * (uint64_t) d->res[1] * (uint64_t) d->res[0];
    if (E.n_keys > ((uint64_t) 1 << 27)) return fail(ctx, at + "more than 2^27 cells x faces x 2 x n_freq");
    set_frequencies(E, d->n_freq, d->wavenumber);
    return alloc_sums(ctx, E, "mer_exitance_fd_create: clearing the map failed", out);
}

int mer_exitance_clear(mer_context *ctx, mer_exitance h) { return clear_sums(ctx, find_recorder(ctx, h, REC_EXITANCE, "mer_exitance_clear")); }

int mer_exitance_destroy(mer_context *ctx, mer_exitance h) { return destroy_sums(ctx, h, find_recorder(ctx, h, REC_EXITANCE, "mer_exitance_destroy")); }

int mer_render_exitance(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_exitance h) {
    const Recorder *E = find_recorder(ctx, h, REC_EXITANCE, "mer_render_exitance", scene != nullptr);
    return E ? launch_exitance(ctx, scene, shard, seed, *E) : 1;
}

int mer_exitance_read(mer_context *ctx, mer_exitance h, double *sums, double totals[16]) {
    const Recorder *E = find_recorder(ctx, h, REC_EXITANCE, "mer_exitance_read");
    if (!E) return 1;
    if (E->fd()) return fail(ctx, "mer_exitance_read: frequency-domain map: use mer_exitance_fd_read");
    return read_sums(ctx, *E, sums, totals, "mer_exitance_read");       // [15] is never written: 0
}

int mer_exitance_fd_read(mer_context *ctx, mer_exitance h, double *sums, double totals[16]) {
    const Recorder *E = find_recorder(ctx, h, REC_EXITANCE, "mer_exitance_fd_read");
    if (!E) return 1;
    if (!E->fd()) return fail(ctx, "mer_exitance_fd_read: steady or time-gated map: use mer_exitance_read");
    return read_sums(ctx, *E, sums, totals, "mer_exitance_fd_read");       // [8..10] and [15] are never written: 0
}

}
