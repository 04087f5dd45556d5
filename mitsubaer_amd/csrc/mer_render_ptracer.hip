// mer_render_ptracer.hip -- the light tracer (integrator = MER_INTEGRATOR_PTRACER): instantiations of K_ptracer (mer_ptracer.hpp), its host
// loop, and the two leaf entry points of the sensor connection.  The light paths of a shard are the (pixel, sample index) pairs K_gen
// would enumerate, launched PT_PATHS_PER_LAUNCH (curved rays: PT_PATHS_PER_LAUNCH_CURVED) at a time on the context stream: no launch runs long, and the film is the only output.
#include "mer_internal.hpp"
#include "mer_ptracer.hpp"

namespace mer {

typedef void (*PtracerKernel)(const Params, uint64_t, uint32_t);

template <bool CURVED, int RIF, int STEPPER> static PtracerKernel pick_sigma(int sigma) {
    return sigma == MER_SIGMA_GRID ? ptracer_kernel<CURVED, RIF, STEPPER, MER_SIGMA_GRID> : ptracer_kernel<CURVED, RIF, STEPPER, MER_SIGMA_HOMOGENEOUS>;
}
template <int RIF> static PtracerKernel pick_curved(int stepper, int sigma) {
    if (stepper == MER_STEP_VERLET) return pick_sigma<true, RIF, MER_STEP_VERLET>(sigma);
    if (stepper == MER_STEP_RK4) return pick_sigma<true, RIF, MER_STEP_RK4>(sigma);
    return nullptr;
}
// a dense trilinear RIF is read with global loads whatever its size (the buffer-load fetch kind is a wavefront-kernel optimisation)
static PtracerKernel pick_ptracer(const mer_scene_desc *sc) {
    const int sigma = sc->sigma_mode == MER_SIGMA_GRID ? MER_SIGMA_GRID : MER_SIGMA_HOMOGENEOUS;
    switch (sc->rif_mode) {
    case MER_RIF_CONST: return pick_sigma<false, MER_RIF_TRILINEAR, MER_STEP_VERLET>(sigma);
    case MER_RIF_TRILINEAR: return pick_curved<MER_RIF_TRILINEAR>(sc->stepper, sigma);
    case MER_RIF_BSPLINE3: return pick_curved<MER_RIF_BSPLINE3>(sc->stepper, sigma);
    case MER_RIF_ACOUSTIC: return pick_curved<RIFK_ACOUSTIC>(sc->stepper, sigma);
    }
    return nullptr;
}

int launch_ptracer(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, float *film_dev, uint64_t n_film) {
    Params P;
    if (make_params(ctx, scene, P, false)) return 1;
    if (scene->integrator != MER_INTEGRATOR_PTRACER) return fail(ctx, "launch_ptracer: the scene's integrator is not ptracer");
    if (!shard || shard->spp_count < 0 || shard->spp_stride <= 0 || shard->tile_count <= 0 || shard->tile_rank < 0 ||
        shard->tile_rank >= shard->tile_count || shard->spp_begin < 0)
        return fail(ctx, "invalid shard");
    if (P.n_point <= 0) return fail(ctx, "ptracer: the scene has no emitter (list entries of kind point, spot or collimated)");
    const PtracerKernel kernel = pick_ptracer(scene);
    if (!kernel) return fail(ctx, "unsupported rif_mode / stepper combination");
    // the work ids of the shard, as launch_render lays them out for K_gen (decode_work)
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
        hipLaunchKernelGGL(kernel, dim3((count + PT_BLOCK - 1) / PT_BLOCK), dim3(PT_BLOCK), 0, ctx->stream, P, first, count);
        HIP_CHECK(ctx, hipGetLastError());
    }
    HIP_CHECK(ctx, hipEventRecord(ctx->ev1, ctx->stream));
    ctx->timed = true;
    HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));                  // mer_render returns synchronised, as the wavefront loop does
    ctx->last_event_ms = 0; ctx->last_march_ms = 0; ctx->last_passes = 0; ctx->last_pipes = 1;
    return 0;
}

// the kernels of the two leaf entry points (here, not in mer_ptracer.hpp: a second translation unit includes that header)
__global__ void sensor_direct_kernel(const Params P, const float *ref, int64_t n, float *out) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float u, v, dist; f3 d;
    const float val = sensor_direct(P, f3(ref[3 * i], ref[3 * i + 1], ref[3 * i + 2]), u, v, d, dist);
    float *o = out + 8 * i;
    o[0] = val; o[1] = u; o[2] = v; o[3] = d.x; o[4] = d.y; o[5] = d.z; o[6] = dist; o[7] = 0.0f;
}
__global__ void sensor_position_kernel(const Params P, const float *dirs, int64_t n, float *uv, int32_t *ok) {
    const int64_t i = (int64_t) blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    float u, v;
    const bool good = sensor_position(P, f3(dirs[3 * i], dirs[3 * i + 1], dirs[3 * i + 2]), u, v);
    uv[2 * i] = u; uv[2 * i + 1] = v; ok[i] = good ? 1 : 0;
}

// the pinhole's sampleDirect / getSamplePosition for the leaf entry points: the scene's sensor fields only
static int sensor_params(mer_context *ctx, const mer_scene_desc *scene, Params &P, const char *who) {
    if (!scene) return fail(ctx, std::string(who) + ": no scene");
    if (scene->sensor != MER_SENSOR_PERSPECTIVE) return fail(ctx, std::string(who) + ": the perspective sensor only");
    mer_scene_desc sc = *scene; sc.sigma_mode = MER_SIGMA_HOMOGENEOUS; sc.rif_mode = MER_RIF_CONST; sc.albedo_mode = MER_ALBEDO_CONST;
    // the light tracer's checks of the sensor (a rigid cam_to_world) apply whatever the scene's integrator is; its emitters are not read
    mer_emitter none{}; none.type = MER_EMITTER_POINT; none.sampling_weight = 1.0f;
    sc.integrator = MER_INTEGRATOR_PTRACER; sc.integrator_reserved = 0;
    sc.emitters = &none; sc.n_emitters = 1;
    for (int i = 0; i < 3; i++) { sc.env_radiance[i] = sc.emission[i] = sc.point_intensity[i] = sc.area_radiance[i] = 0.0f; }
    sc.boundary_bsdf = MER_BSDF_NULL; if (sc.boundary == MER_BOUNDARY_SDF) sc.boundary = MER_BOUNDARY_AABB;
    return make_params(ctx, &sc, P);
}

}  // namespace mer

using namespace mer;

struct PtDevBuf {
    void *p = nullptr;
    ~PtDevBuf() { if (p) (void) hipFree(p); }
};

extern "C" {

int mer_sensor_direct(mer_context *ctx, const mer_scene_desc *scene, const float *ref, int64_t n, float *out) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    Params P;
    if (sensor_params(ctx, scene, P, "mer_sensor_direct")) return 1;
    if (n < 0 || (n > 0 && (!ref || !out))) return fail(ctx, "mer_sensor_direct: invalid arguments");
    if (n == 0) return 0;
    PtDevBuf a, r;
    HIP_CHECK(ctx, hipMalloc(&a.p, (size_t) n * 12)); HIP_CHECK(ctx, hipMalloc(&r.p, (size_t) n * 32));
    HIP_CHECK(ctx, hipMemcpyAsync(a.p, ref, (size_t) n * 12, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(sensor_direct_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P, (const float *) a.p, n, (float *) r.p);
    HIP_CHECK(ctx, hipGetLastError());
    HIP_CHECK(ctx, hipMemcpyAsync(out, r.p, (size_t) n * 32, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

int mer_sensor_position(mer_context *ctx, const mer_scene_desc *scene, const float *dirs, int64_t n, float *out_uv, int32_t *out_ok) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    Params P;
    if (sensor_params(ctx, scene, P, "mer_sensor_position")) return 1;
    if (n < 0 || (n > 0 && (!dirs || !out_uv || !out_ok))) return fail(ctx, "mer_sensor_position: invalid arguments");
    if (n == 0) return 0;
    PtDevBuf a, r, k;
    HIP_CHECK(ctx, hipMalloc(&a.p, (size_t) n * 12)); HIP_CHECK(ctx, hipMalloc(&r.p, (size_t) n * 8)); HIP_CHECK(ctx, hipMalloc(&k.p, (size_t) n * 4));
    HIP_CHECK(ctx, hipMemcpyAsync(a.p, dirs, (size_t) n * 12, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(sensor_position_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P, (const float *) a.p, n, (float *) r.p, (int32_t *) k.p);
    HIP_CHECK(ctx, hipGetLastError());
    HIP_CHECK(ctx, hipMemcpyAsync(out_uv, r.p, (size_t) n * 8, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipMemcpyAsync(out_ok, k.p, (size_t) n * 4, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}

}
