// mer_render_sensitivity.hip -- the sensitivity grids of the detectors on the boundary: instantiations of K_detect and K_replay
// (mer_sensitivity.hpp), the per-chunk loop that runs them back to back (for_light_path_chunks, mer_lightpath_host.hpp) and the
// mer_sensitivity_* entry points, over the Recorder of family REC_SENSITIVITY and what mer_lightpath_host.hpp shares.  The detected-path list
// is the context's: 64 words whose first is the count, then the ids, the three channels of w and the measurements, capacity words each.
#include "mer_lightpath_host.hpp"
#include "mer_sensitivity.hpp"

namespace mer {

struct DetectFamily {
    typedef void (*Kernel)(const Params, const Detector, const DetectList, double *, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return detect_kernel<CURVED, RIF, STEPPER, SIGMA>; }
};
struct ReplayFamily {
    typedef void (*Kernel)(const Params, const FluenceGrid, const DetectList, uint64_t, uint32_t, uint32_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return replay_kernel<CURVED, RIF, STEPPER, SIGMA, false>; }
};
// several measurements or a scattering grid
struct ReplayArrayFamily {
    typedef ReplayFamily::Kernel Kernel;
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return replay_kernel<CURVED, RIF, STEPPER, SIGMA, true>; }
};

// the box and the detector: what mer_sensitivity_create refuses, under the caller's prefix
static int check_sensitivity_desc(mer_context *ctx, const std::string &at, const int32_t res[3], const float bmin[3], const float bmax[3], const mer_detector_desc &t) {
    if (check_box(ctx, at, res, bmin, bmax) || check_raster(ctx, at, "detector res", t, 1)) return 1;
    const int faces = t.boundary == MER_BOUNDARY_SPHERE ? 1 : 6;
    if (t.face < 0 || t.face >= faces) return fail(ctx, at + "face must be one of the boundary's faces (0 ... 5 for the cube, 0 for the sphere)");
    if (t.iu0 < 0 || t.iu1 > t.res[0] || t.iv0 < 0 || t.iv1 > t.res[1]) return fail(ctx, at + "the window must lie inside the raster (0 <= iu0, iu1 <= res[0], 0 <= iv0, iv1 <= res[1])");
    if (!(t.iu0 < t.iu1 && t.iv0 < t.iv1)) return fail(ctx, at + "the window is empty (iu0 < iu1 and iv0 < iv1 are required)");
    return 0;
}
// ... and what the array adds
static int check_sensitivity_array_desc(mer_context *ctx, const mer_sensitivity_array_desc *d) {
    const std::string at = "mer_sensitivity_array_create: ";
    const mer_detector_desc &t = d->det;
    if (check_sensitivity_desc(ctx, at, d->res, d->bmin, d->bmax, t)) return 1;
    if (d->bin_u < 1 || d->bin_v < 1) return fail(ctx, at + "bin_u and bin_v must be at least 1");
    if ((t.iu1 - t.iu0) % d->bin_u || (t.iv1 - t.iv0) % d->bin_v) return fail(ctx, at + "bin_u and bin_v must divide the window (iu1 - iu0 and iv1 - iv0)");
    if (d->gates < 1) return fail(ctx, at + "gates must be at least 1");
    if (d->gates > 1 && t.t_bin == 0) return fail(ctx, at + "several gates need t_bin > 0");
    if (d->scatter != 0 && d->scatter != 1) return fail(ctx, at + "scatter must be 0 or 1");
    if (d->reserved[0] != 0 || d->reserved[1] != 0) return fail(ctx, at + "reserved must be 0");
    const uint64_t cells = (uint64_t) d->res[0] * (uint64_t) d->res[1] * (uint64_t) d->res[2];
    const uint64_t grids = (uint64_t) (1 + d->scatter) * (uint64_t) d->gates * (uint64_t) ((t.iu1 - t.iu0) / d->bin_u) * (uint64_t) ((t.iv1 - t.iv0) / d->bin_v);
    if (grids > ((uint64_t) 1 << 27) || grids * cells > ((uint64_t) 1 << 27)) return fail(ctx, at + "more than 2^27 cells x measurements x (1 + scatter)");
    return 0;
}

// the Recorder of a checked description
static int create_sensitivity(mer_context *ctx, const int32_t res[3], const float bmin[3], const float bmax[3], const mer_detector_desc &t, int32_t bin_u,
                              int32_t bin_v, int32_t gates, int32_t scatter, const std::string &clearing_failed, mer_sensitivity *out) {
    Recorder J;
    J.family = REC_SENSITIVITY; J.n_totals = SENS_TOTALS; J.det = t;
    for (int a = 0; a < 3; a++) { J.box.res[a] = res[a]; J.box.bmin[a] = bmin[a]; J.box.bmax[a] = bmax[a]; }
    J.bin_u = bin_u; J.bin_v = bin_v; J.gates = gates; J.scatter = scatter;
    J.n_meas = (uint64_t) gates * (uint64_t) ((t.iv1 - t.iv0) / bin_v) * (uint64_t) ((t.iu1 - t.iu0) / bin_u);
    J.n_keys = (uint64_t) (1 + scatter) * J.n_meas * J.n_cells();
    return alloc_sums(ctx, J, clearing_failed, out);
}

// the context's list, grown to hold `cap` records
static int detect_list(mer_context *ctx, uint32_t cap, DetectList &L) {
    if (ctx->detect_cap < cap) {
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
        ctx->detect_cap = 0;
        if (ctx->detect_list.reserve(ctx, (DETECT_HEAD + (size_t) cap * 5) * sizeof(uint32_t))) return 1;
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
    const ReplayFamily::Kernel replay = J.n_meas > 1 || J.scatter ? pick_light_kernel<ReplayArrayFamily>(scene) : pick_light_kernel<ReplayFamily>(scene);
    if (!detect || !replay) return fail(ctx, "unsupported rif_mode / stepper combination");
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    DetectList L;
    if (detect_list(ctx, scene->rif_mode == MER_RIF_CONST ? PT_PATHS_PER_LAUNCH : PT_PATHS_PER_LAUNCH_CURVED, L)) return 1;
    Detector D;
    D.res_u = t.res[0]; D.res_v = t.res[1]; D.t_min = t.t_min; D.t_bin = t.t_bin; D.cos_min = t.cos_min;
    D.face = t.face; D.iu0 = t.iu0; D.iu1 = t.iu1; D.iv0 = t.iv0; D.iv1 = t.iv1;
    D.bins = (uint32_t) J.bin_u | (uint32_t) J.bin_v << 16; D.gates = J.gates;       // bins of at most 4096 cells
    const FluenceGrid G = fluence_grid<FluenceGrid>(ctx, J);
    double *totals = J.totals();                             // the measurements follow them (Recorder::meas)
    const uint32_t n_meas = (uint32_t) J.n_meas, scatter = (uint32_t) J.scatter;
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
        hipLaunchKernelGGL(replay, dim3((detected + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, ctx->stream, P, G, L, first, detected, n_meas, scatter);
        HIP_CHECK(ctx, hipGetLastError());
        return 0;
    });
}

}  // namespace mer

using namespace mer;

extern "C" {

int mer_sensitivity_create(mer_context *ctx, const mer_sensitivity_desc *d, mer_sensitivity *out) {
    if (!create_args(ctx, d, out, "mer_sensitivity_create") || check_sensitivity_desc(ctx, "mer_sensitivity_create: ", d->res, d->bmin, d->bmax, d->det)) return 1;
    // one detector: the whole window, one gate
    return create_sensitivity(ctx, d->res, d->bmin, d->bmax, d->det, d->det.iu1 - d->det.iu0, d->det.iv1 - d->det.iv0, 1, 0,
                              "mer_sensitivity_create: clearing the grid failed", out);
}

int mer_sensitivity_array_create(mer_context *ctx, const mer_sensitivity_array_desc *d, mer_sensitivity *out) {
    if (!create_args(ctx, d, out, "mer_sensitivity_array_create") || check_sensitivity_array_desc(ctx, d)) return 1;
    return create_sensitivity(ctx, d->res, d->bmin, d->bmax, d->det, d->bin_u, d->bin_v, d->gates, d->scatter,
                              "mer_sensitivity_array_create: clearing the grids failed", out);
}

int mer_sensitivity_clear(mer_context *ctx, mer_sensitivity h) { return clear_sums(ctx, find_recorder(ctx, h, REC_SENSITIVITY, "mer_sensitivity_clear")); }

int mer_sensitivity_destroy(mer_context *ctx, mer_sensitivity h) { return destroy_sums(ctx, h, find_recorder(ctx, h, REC_SENSITIVITY, "mer_sensitivity_destroy")); }

int mer_render_sensitivity(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, mer_sensitivity h) {
    const Recorder *J = find_recorder(ctx, h, REC_SENSITIVITY, "mer_render_sensitivity", scene != nullptr);
    return J ? launch_sensitivity(ctx, scene, shard, seed, *J) : 1;
}

int mer_sensitivity_read(mer_context *ctx, mer_sensitivity h, double *sums, double totals[16]) {
    const Recorder *J = find_recorder(ctx, h, REC_SENSITIVITY, "mer_sensitivity_read");
    if (!J) return 1;
    if (J->n_meas > 1 || J->scatter) return fail(ctx, "mer_sensitivity_read: the handle holds several measurements or a scattering grid: use mer_sensitivity_read_array");
    return read_sums(ctx, *J, sums, totals, "mer_sensitivity_read");       // [13..15] are written with scatter only: 0
}

int mer_sensitivity_shape(mer_context *ctx, mer_sensitivity h, int32_t shape[4]) {
    const Recorder *J = find_recorder(ctx, h, REC_SENSITIVITY, "mer_sensitivity_shape");
    if (!J) return 1;
    if (!shape) return fail(ctx, "mer_sensitivity_shape: invalid arguments");
    shape[0] = J->gates; shape[1] = (J->det.iv1 - J->det.iv0) / J->bin_v; shape[2] = (J->det.iu1 - J->det.iu0) / J->bin_u; shape[3] = J->scatter;
    return 0;
}

int mer_sensitivity_read_array(mer_context *ctx, mer_sensitivity h, double *sums, double *meas, double totals[16]) {
    const Recorder *J = find_recorder(ctx, h, REC_SENSITIVITY, "mer_sensitivity_read_array");
    if (!J || read_sums(ctx, *J, sums, totals, "mer_sensitivity_read_array")) return 1;
    if (meas) HIP_CHECK(ctx, hipMemcpy(meas, J->meas(), (size_t) J->n_meas * MEAS_WORDS * sizeof(double), hipMemcpyDeviceToHost));
    return 0;
}

}
