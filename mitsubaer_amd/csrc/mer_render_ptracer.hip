// mer_render_ptracer.hip -- the light tracer (integrator = MER_INTEGRATOR_PTRACER): instantiations of K_ptracer (mer_ptracer.hpp), its launch
// (launch_light_paths, mer_lightpath_host.hpp: the film is the only output), and the two leaf entry points of the sensor connection.
#include "mer_lightpath_host.hpp"
#include "mer_ptracer.hpp"

namespace mer {

struct PtracerFamily {
    typedef void (*Kernel)(const Params, uint64_t, uint32_t);
    template <bool CURVED, int RIF, int STEPPER, int SIGMA> static Kernel get() { return ptracer_kernel<CURVED, RIF, STEPPER, SIGMA>; }
};

int launch_ptracer(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, float *film_dev, uint64_t n_film) {
    Params P;
    if (make_params(ctx, scene, P, false)) return 1;
    if (scene->integrator != MER_INTEGRATOR_PTRACER) return fail(ctx, "launch_ptracer: the scene's integrator is not ptracer");
    if (check_light_paths(ctx, scene, shard, P)) return 1;
    return launch_light_paths(ctx, scene, P, seed, film_dev, n_film, pick_light_kernel<PtracerFamily>(scene));
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
    mer_scene_desc sc = sensor_fields_only(*scene);
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

extern "C" {

int mer_sensor_direct(mer_context *ctx, const mer_scene_desc *scene, const float *ref, int64_t n, float *out) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    Params P;
    if (sensor_params(ctx, scene, P, "mer_sensor_direct")) return 1;
    if (n < 0 || (n > 0 && (!ref || !out))) return fail(ctx, "mer_sensor_direct: invalid arguments");
    if (n == 0) return 0;
    DeviceBuffer a, r;
    if (a.alloc(ctx, (size_t) n * 12) || r.alloc(ctx, (size_t) n * 32)) return 1;
    HIP_CHECK(ctx, hipMemcpyAsync(a.p, ref, (size_t) n * 12, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(sensor_direct_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P, a.as<const float>(), n, r.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return r.download(ctx, out, (size_t) n * 32);
}

int mer_sensor_position(mer_context *ctx, const mer_scene_desc *scene, const float *dirs, int64_t n, float *out_uv, int32_t *out_ok) {
    if (!ctx) return 1;
    (void) hipSetDevice(ctx->device);
    Params P;
    if (sensor_params(ctx, scene, P, "mer_sensor_position")) return 1;
    if (n < 0 || (n > 0 && (!dirs || !out_uv || !out_ok))) return fail(ctx, "mer_sensor_position: invalid arguments");
    if (n == 0) return 0;
    DeviceBuffer a, r, k;
    if (a.alloc(ctx, (size_t) n * 12) || r.alloc(ctx, (size_t) n * 8) || k.alloc(ctx, (size_t) n * 4)) return 1;
    HIP_CHECK(ctx, hipMemcpyAsync(a.p, dirs, (size_t) n * 12, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL(sensor_position_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P, a.as<const float>(), n, r.as<float>(), k.as<int32_t>());
    HIP_CHECK(ctx, hipGetLastError());
    HIP_CHECK(ctx, hipMemcpyAsync(out_uv, r.p, (size_t) n * 8, hipMemcpyDeviceToHost, ctx->stream));
    return k.download(ctx, out_ok, (size_t) n * 4);
}

}
