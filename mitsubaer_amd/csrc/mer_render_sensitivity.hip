// mer_render_sensitivity.hip -- the sensitivity grid of a detector on the boundary: instantiations of K_detect and K_replay
// (mer_sensitivity.hpp), the per-chunk loop that runs them back to back (for_light_path_chunks, mer_lightpath_host.hpp) and the
// mer_sensitivity_* entry points, over the Recorder of family REC_SENSITIVITY and what mer_lightpath_host.hpp shares.  The detected-path list
// is the context's: 64 words whose first is the count, then the ids and the three channels of w, capacity words each.
#include "mer_lightpath_host.hpp"
#include "mer_sensitivity.hpp"

namespace mer {

struct DetectFamily {
    typedef void (*Kernel)(const Params, const Detector, const DetectList, double *, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return detect_kernel<CURVED, RIF, STEPPER, SIGMA>; }
};
struct ReplayFamily {
    typedef void (*Kernel)(const Params, const FluenceGrid, const DetectList, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return replay_kernel<CURVED, RIF, STEPPER, SIGMA>; }
};

static int check_sensitivity_desc(mer_context *ctx, const mer_sensitivity_desc *d) {
    const std::string at = "mer_sensitivity_create: ";
    const mer_detector_desc &t = d->det;
    if (check_box(ctx, at, d->res, d->bmin, d->bmax) || check_raster(ctx, at, "detector res", t, 1)) return 1;
    const int faces = t.boundary == MER_BOUNDARY_SPHERE ? 1 : 6;
    if (t.face < 0 || t.face >= faces) return fail(ctx, at + "face must be one of the boundary's faces (0 ... 5 for the cube, 0 for the sphere)");
    if (t.iu0 < 0 || t.iu1 > t.res[0] || t.iv0 < 0 || t.iv1 > t.res[1]) return fail(ctx, at + "the window must lie inside the raster (0 <= iu0, iu1 <= res[0], 0 <= iv0, iv1 <= res[1])");
    if (!(t.iu0 < t.iu1 && t.iv0 < t.iv1)) return fail(ctx, at + "the window is empty (iu0 < iu1 and iv0 < iv1 are required)");
    return 0;
}

// the context's list, grown to hold `cap` records
static int detect_list(mer_context *ctx, uint32_t cap, DetectList &L) {
    if (ctx->detect_cap < cap) {
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->detect_cap = 0;
        if (ctx->detect_list.reserve(ctx, (DETECT_HEAD + (size_t) cap * 4) * sizeof(uint32_t))) return 1;
        ctx->detect_cap = cap;
    }
    L.count = ctx->detect_list.as<uint32_t>();
    L.cap = ctx->detect_cap; L.chk = ctx->chk;
    return 0;
}

static int launch_sensitivity(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, const Recorder &J) {
    Params P;
    if (open_light_paths(ctx, scene, shard, J, P, "mer_render_sensitivity: the scene's integrator must be ptracer (the grid is recorded from light paths)",
                         "mer_render_sensitivity: the scene's boundary differs from the detector's (a cube has 6 faces, a sphere 1)")) return 1;
    const mer_detector_desc &t = J.det;
    const DetectFamily::Kernel detect = pick_light_kernel<DetectFamily>(scene);
    const ReplayFamily::Kernel replay = pick_light_kernel<ReplayFamily>(scene);
    if (!detect || !replay) return fail(ctx, "unsupported rif_mode / stepper combination");
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DetectList L;
    if (detect_list(ctx, scene->rif_mode == MER_RIF_CONST ? PT_PATHS_PER_LAUNCH : PT_PATHS_PER_LAUNCH_CURVED, L)) return 1;
    Detector D;
    D.res_u = t.res[0]; D.res_v = t.res[1]; D.t_min = t.t_min; D.t_bin = t.t_bin; D.cos_min = t.cos_min;
    D.face = t.face; D.iu0 = t.iu0; D.iu1 = t.iu1; D.iv0 = t.iv0; D.iv1 = t.iv1;
    const FluenceGrid G = fluence_grid<FluenceGrid>(ctx, J);
    double *totals = J.totals();
    return for_light_path_chunks(ctx, scene, P, seed, nullptr, 0, [&](uint64_t first, uint32_t count) {
        if (count > L.cap) return fail(ctx, "mer_render_sensitivity: a launch chunk exceeds the detected-path list");
        // the count this chunk's second pass is sized by is read back after this chunk's first pass, into a variable that starts at 0
        uint32_t detected = 0;
        HIP_CHECK(ctx, hipMemsetAsync(L.count, 0, sizeof(uint32_t), ctx->stream));
        hipLaunchKernelGGL(detect, dim3((count + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, ctx->stream, P, D, L, totals, first, count);
        HIP_CHECK(ctx, hipGetLastError());
        HIP_CHECK(ctx, hipMemcpyAsync(&detected, L.count, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream));
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (detected > count) return fail(ctx, "mer_render_sensitivity: the detected-path list holds more records than the chunk has paths");
        if (detected == 0) return 0;
        hipLaunchKernelGGL(replay, dim3((detected + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, ctx->stream, P, G, L, first, detected);
        HIP_CHECK(ctx, hipGetLastError());
        return 0;
    });
}

}  // namespace mer

using namespace mer;

extern "C" {

int mer_sensitivity_create(mer_context *ctx, const mer_sensitivity_desc *d, mer_sensitivity *out) {
    if (!create_args(ctx, d, out, "mer_sensitivity_create") || check_sensitivity_desc(ctx, d)) return 1;
    Recorder J;
    J.family = REC_SENSITIVITY; J.n_totals = 16; J.det = d->det;
    for (int a = 0; a < 3; a++) { J.box.res[a] = d->res[a]; J.box.bmin[a] = d->bmin[a]; J.box.bmax[a] = d->bmax[a]; }
    J.n_keys = J.n_cells();
    return alloc_sums(ctx, J, "mer_sensitivity_create: clearing the grid failed", out);
}

int mer_sensitivity_clear(mer_context *ctx, mer_sensitivity h) { return clear_sums(ctx, find_recorder(ctx, h, REC_SENSITIVITY, "mer_sensitivity_clear")); }

int mer_sensitivity_destroy(mer_context *ctx, mer_sensitivity h) { return destroy_sums(ctx, h, find_recorder(ctx, h, REC_SENSITIVITY, "mer_sensitivity_destroy")); }

int mer_render_sensitivity(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_sensitivity h) {
    const Recorder *J = find_recorder(ctx, h, REC_SENSITIVITY, "mer_render_sensitivity", scene != nullptr);
    return J ? launch_sensitivity(ctx, scene, shard, seed, *J) : 1;
}

int mer_sensitivity_read(mer_context *ctx, mer_sensitivity h, double *sums, double totals[16]) {
    const Recorder *J = find_recorder(ctx, h, REC_SENSITIVITY, "mer_sensitivity_read");
    return J ? read_sums(ctx, *J, sums, totals, "mer_sensitivity_read") : 1;       // [13..15] are never written: 0
}

}
