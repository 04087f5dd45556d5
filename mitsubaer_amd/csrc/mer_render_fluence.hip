// mer_render_fluence.hip -- the fluence grid recorded from light paths: instantiations of K_fluence (mer_fluence.hpp), its launch and the
// mer_fluence_* entry points, over the Recorder of family REC_FLUENCE and what mer_lightpath_host.hpp shares.  A time-resolved grid
// (mer_fluence_time_create) renders with the TIMED instantiations, a track-length grid (mer_fluence_track_create) with K_fluence_track
// (mer_render_fluence_track.hip), a frequency-domain grid (mer_fluence_fd_create) with the FD instantiations (mer_render_fluence_fd.hip).
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
// mer_render_fluence_fd.hip: ... and of the frequency-domain kind of K_fluence, for a handle of mer_fluence_fd_create
FluenceKernel pick_fluence_fd(const mer_scene_desc *sc);

// the box checks of mer_fluence_create, then the window's
static int check_fluence_time_desc(mer_context *ctx, const mer_fluence_time_desc *d) {
    const std::string at = "mer_fluence_time_create: ";
    if (check_box(ctx, at, d->res, d->bmin, d->bmax)) return 1;
    if (d->frames < 1 || d->frames > 4096) return fail(ctx, at + "frames must lie in 1 ... 4096");
    if (!std::isfinite(d->t_min)) return fail(ctx, at + "t_min must be finite");
    if (!std::isfinite(d->t_bin) || !(d->t_bin > 0)) return fail(ctx, at + "t_bin must be finite and greater than 0");
    if (d->reserved != 0) return fail(ctx, at + "reserved must be 0");
    const uint64_t cells = (uint64_t) d->res[0] * (uint64_t) d->res[1] * (uint64_t) d->res[2];
    if (cells * (uint64_t) d->frames > ((uint64_t) 1 << 27)) return fail(ctx, at + "more than 2^27 cells x frames");
    return 0;
}

// the grid of a checked box (and window: frames > 0), zeroed, and its handle
// wavenumber (n_freq > 0): a frequency-domain grid, 2 n_freq planes and no window
static int alloc_fluence(mer_context *ctx, const char *who, int kind, const int32_t res[3], const float bmin[3], const float bmax[3], int32_t frames,
                         float t_min, float t_bin, mer_fluence *out, int32_t n_freq = 0, const double *wavenumber = nullptr) {
    Recorder F;
    F.family = REC_FLUENCE; F.kind = kind;
    for (int a = 0; a < 3; a++) { F.box.res[a] = res[a]; F.box.bmin[a] = bmin[a]; F.box.bmax[a] = bmax[a]; }
    F.frames = frames; F.det.t_min = t_min; F.det.t_bin = t_bin;
    F.n_keys = F.n_cells() * (uint64_t) (n_freq > 0 ? 2 * n_freq : frames > 0 ? frames : 1);
    F.n_totals = frames > 0 ? 12 : 8;
    if (n_freq > 0) set_frequencies(F, n_freq, wavenumber);
    return alloc_sums(ctx, F, std::string(who) + ": clearing the grid failed", out);
}

static int launch_fluence(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, const Recorder &F) {
    Params P;
    if (open_light_paths(ctx, scene, shard, F, P, "mer_render_fluence: the scene's integrator must be ptracer (the grid is recorded from light paths)", nullptr)) return 1;
    if (F.track() && scene->sigma_mode != MER_SIGMA_GRID) {
        // the track-length weight is built for ANALOG distance sampling: every free flight drawn from one exponential exp(-rho s)
        const std::string at = "mer_render_fluence: a track-length grid needs analog distance sampling (one exponential per free flight): ";
        if (P.medium_sampling_weight != 1.0f) return fail(ctx, at + "medium_sampling_weight must be 1");
        if (scene->strategy == MER_STRATEGY_MAXIMUM) return fail(ctx, at + "strategy maximum samples the maximum of three exponentials");
        if (scene->strategy == MER_STRATEGY_BALANCE && !(P.sigT.x == P.sigT.y && P.sigT.y == P.sigT.z))
            return fail(ctx, at + "strategy balance with a channel-dependent sigma_t samples a mixture of exponentials");
    }
    const FluenceKernel kernel = F.fd() ? pick_fluence_fd(scene) : F.track() ? pick_fluence_track(scene) : F.timed() ? pick_light_kernel<FluenceFamily<true>>(scene) : pick_light_kernel<FluenceFamily<false>>(scene);
    return launch_light_paths(ctx, scene, P, seed, nullptr, 0, kernel, fluence_grid<FluenceGrid>(ctx, F));
}

}  // namespace mer

using namespace mer;

extern "C" {

int mer_fluence_create(mer_context *ctx, const mer_fluence_desc *d, mer_fluence *out) {
    if (!create_args(ctx, d, out, "mer_fluence_create") || check_box(ctx, "mer_fluence_create: ", d->res, d->bmin, d->bmax)) return 1;
    return alloc_fluence(ctx, "mer_fluence_create", REC_COLLISION, d->res, d->bmin, d->bmax, 0, 0, 0, out);
}

int mer_fluence_track_create(mer_context *ctx, const mer_fluence_desc *d, mer_fluence *out) {
    if (!create_args(ctx, d, out, "mer_fluence_track_create") || check_box(ctx, "mer_fluence_track_create: ", d->res, d->bmin, d->bmax)) return 1;
    return alloc_fluence(ctx, "mer_fluence_track_create", REC_TRACK, d->res, d->bmin, d->bmax, 0, 0, 0, out);
}

int mer_fluence_time_create(mer_context *ctx, const mer_fluence_time_desc *d, mer_fluence *out) {
    if (!create_args(ctx, d, out, "mer_fluence_time_create") || check_fluence_time_desc(ctx, d)) return 1;
    return alloc_fluence(ctx, "mer_fluence_time_create", REC_TIMED, d->res, d->bmin, d->bmax, d->frames, d->t_min, d->t_bin, out);
}

int mer_fluence_fd_create(mer_context *ctx, const mer_fluence_fd_desc *d, mer_fluence *out) {
    const std::string at = "mer_fluence_fd_create: ";
    if (!create_args(ctx, d, out, "mer_fluence_fd_create") || check_box(ctx, at, d->res, d->bmin, d->bmax) ||
        check_frequencies(ctx, at, d->n_freq, d->wavenumber, d->reserved, 2)) return 1;
    if ((uint64_t) d->res[0] * (uint64_t) d->res[1] * (uint64_t) d->res[2] * (uint64_t) (2 * d->n_freq) > ((uint64_t) 1 << 27))
        return fail(ctx, at + "more than 2^27 cells x 2 x n_freq");
    return alloc_fluence(ctx, "mer_fluence_fd_create", REC_FD, d->res, d->bmin, d->bmax, 0, 0, 0, out, d->n_freq, d->wavenumber);
}

int mer_fluence_clear(mer_context *ctx, mer_fluence h) { return clear_sums(ctx, find_recorder(ctx, h, REC_FLUENCE, "mer_fluence_clear")); }

int mer_fluence_destroy(mer_context *ctx, mer_fluence h) { return destroy_sums(ctx, h, find_recorder(ctx, h, REC_FLUENCE, "mer_fluence_destroy")); }

int mer_render_fluence(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_fluence h) {
    const Recorder *F = find_recorder(ctx, h, REC_FLUENCE, "mer_render_fluence", scene != nullptr);
    return F ? launch_fluence(ctx, scene, shard, seed, *F) : 1;
}

int mer_fluence_read(mer_context *ctx, mer_fluence h, double *sums, double totals[8]) {
    const Recorder *F = find_recorder(ctx, h, REC_FLUENCE, "mer_fluence_read");
    if (!F) return 1;
    if (F->timed()) return fail(ctx, "mer_fluence_read: time-resolved grid: use mer_fluence_time_read");
    if (F->fd()) return fail(ctx, "mer_fluence_read: frequency-domain grid: use mer_fluence_fd_read");
    return read_sums(ctx, *F, sums, totals, "mer_fluence_read");
}

int mer_fluence_time_read(mer_context *ctx, mer_fluence h, double *sums, double totals[12]) {
    const Recorder *F = find_recorder(ctx, h, REC_FLUENCE, "mer_fluence_time_read");
    if (!F) return 1;
    if (F->fd()) return fail(ctx, "mer_fluence_time_read: frequency-domain grid: use mer_fluence_fd_read");
    if (!F->timed()) return fail(ctx, "mer_fluence_time_read: steady-state grid: use mer_fluence_read");
    return read_sums(ctx, *F, sums, totals, "mer_fluence_time_read");       // [11] is never written: 0
}

int mer_fluence_fd_read(mer_context *ctx, mer_fluence h, double *sums, double totals[8]) {
    const Recorder *F = find_recorder(ctx, h, REC_FLUENCE, "mer_fluence_fd_read");
    if (!F) return 1;
    if (F->timed()) return fail(ctx, "mer_fluence_fd_read: time-resolved grid: use mer_fluence_time_read");
    if (!F->fd()) return fail(ctx, "mer_fluence_fd_read: steady-state grid: use mer_fluence_read");
    return read_sums(ctx, *F, sums, totals, "mer_fluence_fd_read");
}

}
