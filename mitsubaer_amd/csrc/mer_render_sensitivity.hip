// mer_render_sensitivity.hip -- the sensitivity grid of a detector on the boundary: instantiations of K_detect and K_replay
// (mer_sensitivity.hpp), the per-chunk loop that runs them back to back (for_light_path_chunks, mer_lightpath_host.hpp) and the
// mer_sensitivity_* entry points.  A grid is one device allocation: double[nz][ny][nx][3] sums, then the 16 totals.  The detected-path list
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
    mer_fluence_desc box;
    for (int a = 0; a < 3; a++) { box.res[a] = d->res[a]; box.bmin[a] = d->bmin[a]; box.bmax[a] = d->bmax[a]; }
    if (check_fluence_desc(ctx, &box, at)) return 1;
    const mer_detector_desc &t = d->det;
    if (t.boundary != MER_BOUNDARY_AABB && t.boundary != MER_BOUNDARY_SPHERE) return fail(ctx, at + "boundary must be the cube (MER_BOUNDARY_AABB) or the sphere (MER_BOUNDARY_SPHERE)");
    for (int a = 0; a < 2; a++)
        if (t.res[a] < 1 || t.res[a] > 4096) return fail(ctx, at + "detector res must lie in 1 ... 4096 on both axes");
    if (!std::isfinite(t.t_bin) || t.t_bin < 0) return fail(ctx, at + "t_bin must be finite and at least 0");
    if (!std::isfinite(t.t_min)) return fail(ctx, at + "t_min must be finite");
    if (!(t.cos_min >= 0 && t.cos_min < 1)) return fail(ctx, at + "cos_min must lie in 0 <= cos_min < 1");
    if (t.reserved != 0) return fail(ctx, at + "reserved must be 0");
    const int faces = t.boundary == MER_BOUNDARY_SPHERE ? 1 : 6;
    if (t.face < 0 || t.face >= faces) return fail(ctx, at + "face must be one of the boundary's faces (0 ... 5 for the cube, 0 for the sphere)");
    if (t.iu0 < 0 || t.iu1 > t.res[0] || t.iv0 < 0 || t.iv1 > t.res[1]) return fail(ctx, at + "the window must lie inside the raster (0 <= iu0, iu1 <= res[0], 0 <= iv0, iv1 <= res[1])");
    if (!(t.iu0 < t.iu1 && t.iv0 < t.iv1)) return fail(ctx, at + "the window is empty (iu0 < iu1 and iv0 < iv1 are required)");
    return 0;
}

static Sensitivity *find_sensitivity(mer_context *ctx, mer_sensitivity h, const char *who) { return find_sums(ctx, ctx->sensitivities, h, who, "sensitivity"); }

// the context's list, grown to hold `cap` records
static int detect_list(mer_context *ctx, uint32_t cap, DetectList &L) {
    if (ctx->detect_cap < cap) {
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        if (ctx->detect_list) (void) hipFree(ctx->detect_list);
        ctx->detect_list = nullptr; ctx->detect_cap = 0;
        HIP_CHECK(ctx, hipMalloc((void **) &ctx->detect_list, (DETECT_HEAD + (size_t) cap * 4) * sizeof(uint32_t)));
        ctx->detect_cap = cap;
    }
    L.count = ctx->detect_list;
    L.cap = ctx->detect_cap; L.chk = ctx->chk;
    return 0;
}

static int launch_sensitivity(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, const Sensitivity &J) {
    if (scene->integrator != MER_INTEGRATOR_PTRACER)
        return fail(ctx, "mer_render_sensitivity: the scene's integrator must be ptracer (the grid is recorded from light paths)");
    Params P;
    if (make_params(ctx, scene, P, false)) return 1;
    const mer_detector_desc &t = J.desc.det;
    if (scene->boundary != t.boundary)
        return fail(ctx, "mer_render_sensitivity: the scene's boundary differs from the detector's (a cube has 6 faces, a sphere 1)");
    if (check_light_paths(ctx, P, shard)) return 1;
    const DetectFamily::Kernel detect = pick_light_kernel<DetectFamily>(scene);
    const ReplayFamily::Kernel replay = pick_light_kernel<ReplayFamily>(scene);
    if (!detect || !replay) return fail(ctx, "unsupported rif_mode / stepper combination");
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DetectList L;
    if (detect_list(ctx, scene->rif_mode == MER_RIF_CONST ? PT_PATHS_PER_LAUNCH : PT_PATHS_PER_LAUNCH_CURVED, L)) return 1;
    Detector D;
    D.res_u = t.res[0]; D.res_v = t.res[1]; D.t_min = t.t_min; D.t_bin = t.t_bin; D.cos_min = t.cos_min;
    D.face = t.face; D.iu0 = t.iu0; D.iu1 = t.iu1; D.iv0 = t.iv0; D.iv1 = t.iv1;
    FluenceGrid G;
    G.sums = J.dev; G.totals = J.totals(); G.chk = ctx->chk; G.n_cells = J.n_keys();
    G.frames = 0; G.t_min = 0; G.t_bin = 0;
    for (int a = 0; a < 3; a++) { G.res[a] = J.desc.res[a]; G.bmin[a] = J.desc.bmin[a]; G.bmax[a] = J.desc.bmax[a]; }
    double *totals = J.totals();
    return for_light_path_chunks(ctx, scene, P, shard, seed, nullptr, 0, [&](uint64_t first, uint32_t count) {
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

int mer_sensitivity_create(mer_context *ctx, const mer_sensitivity_desc *desc, mer_sensitivity *out) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    if (!desc || !out) return fail(ctx, "mer_sensitivity_create: invalid arguments");
    *out = 0;
    if (check_sensitivity_desc(ctx, desc)) return 1;
    Sensitivity J;
    J.desc = *desc;
    return alloc_sums(ctx, ctx->sensitivities, J, "mer_sensitivity_create: clearing the grid failed", out);
}

int mer_sensitivity_clear(mer_context *ctx, mer_sensitivity h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Sensitivity *J = find_sensitivity(ctx, h, "mer_sensitivity_clear");
    if (!J) return 1;
    return clear_sums(ctx, *J);
}

int mer_sensitivity_destroy(mer_context *ctx, mer_sensitivity h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Sensitivity *J = find_sensitivity(ctx, h, "mer_sensitivity_destroy");
    if (!J) return 1;
    return destroy_sums(ctx, ctx->sensitivities, h, *J);
}

int mer_render_sensitivity(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_sensitivity h) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    if (!scene) return fail(ctx, "mer_render_sensitivity: no scene");
    const Sensitivity *J = find_sensitivity(ctx, h, "mer_render_sensitivity");
    if (!J) return 1;
    return launch_sensitivity(ctx, scene, shard, seed, *J);
}

int mer_sensitivity_read(mer_context *ctx, mer_sensitivity h, double *sums, double totals[16]) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    const Sensitivity *J = find_sensitivity(ctx, h, "mer_sensitivity_read");
    if (!J) return 1;
    if (!totals) return fail(ctx, "mer_sensitivity_read: invalid arguments");
    return read_sums(ctx, *J, sums, totals, 16);       // [13..15] are never written: 0
}

}
