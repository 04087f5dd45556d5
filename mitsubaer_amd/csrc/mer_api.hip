// mer_api.hip -- libmer.so: C-ABI (include/mer.h) over the gfx950 kernels in mer_kernels.hpp: the context and its options, volumes,
// envmap upload, film, render entry points and the leaf calls.  A scene becomes kernel arguments in mer_scene.hip (make_params).
// Host side is plain HIP runtime: device memory, one stream, HIP events.  No CPU compute path exists:
// every entry point that computes launches a kernel, and fails loudly when no device is present.
#include "mer_internal.hpp"
// every entry point runs on its context's device: a process may hold contexts of several GPUs (mer_multi.hip), and the current device is per-thread state
#define MER_USE_DEVICE(ctx) do { if (ctx) (void) hipSetDevice((ctx)->device); } while (0)
#include "mer_kernels.hpp"
#include <algorithm>
#include <functional>
#include <utility>

using namespace mer;

namespace { thread_local std::string g_create_error; }

namespace mer {

// The fetch kinds and steppers the curved-ray leaf kernels are instantiated for, and a run-time value as the std::integral_constant of
// the listed one it equals: returns f(constant), or false when the value is none of them.
using FetchKinds = std::integer_sequence<int, RIFK_ACOUSTIC, MER_RIF_TRILINEAR, RIFK_DENSE_BUF, RIFK_CELL8, RIFK_CELL8_BUF, RIFK_BRICK27_BUF, RIFK_BRICK27, MER_RIF_BSPLINE3>;
using Steppers = std::integer_sequence<int, MER_STEP_VERLET, MER_STEP_RK4>;
template <int... Ks, typename F> static bool match_constant(std::integer_sequence<int, Ks...>, int value, F &&f) {
    return ((value == Ks && f(std::integral_constant<int, Ks>())) || ...);
}

template <typename F> static int dispatch_modes(mer_context *ctx, const mer_scene_desc *sc, F &&f) {
    const bool curved = sc->rif_mode != MER_RIF_CONST;
    const bool grid = sc->sigma_mode == MER_SIGMA_GRID;
    if (!curved) {
        if (grid) return f(std::integral_constant<bool, false>(), std::integral_constant<int, MER_RIF_TRILINEAR>(),
                           std::integral_constant<int, MER_STEP_VERLET>(), std::integral_constant<int, MER_SIGMA_GRID>(), std::integral_constant<int, 0>());
        return f(std::integral_constant<bool, false>(), std::integral_constant<int, MER_RIF_TRILINEAR>(),
                 std::integral_constant<int, MER_STEP_VERLET>(), std::integral_constant<int, MER_SIGMA_HOMOGENEOUS>(), std::integral_constant<int, 0>());
    }
    // internal fetch kind of the trilinear RIF (mer_device.hpp): layout x {global, buffer} loads
    int rc = 0;
    const bool known = match_constant(FetchKinds(), rif_fetch_kind(ctx, sc), [&](auto rif) {
        return match_constant(Steppers(), sc->stepper, [&](auto stepper) {
            rc = grid ? f(std::integral_constant<bool, true>(), rif, stepper, std::integral_constant<int, MER_SIGMA_GRID>(), std::integral_constant<int, 0>())
                      : f(std::integral_constant<bool, true>(), rif, stepper, std::integral_constant<int, MER_SIGMA_HOMOGENEOUS>(), std::integral_constant<int, 0>());
            return true;
        });
    });
    if (known) return rc;
    return fail(ctx, "unsupported rif_mode / stepper combination");
}
}  // namespace mer

extern "C" {

int mer_abi_version(void) { return MER_ABI_VERSION; }

int mer_context_create(int32_t device_id, mer_context **out) {
    if (!out) return 1;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_create_error = "mer_context_create: no HIP device available (libmer has no CPU path)";
        return 1;
    }
    if (device_id < 0 || device_id >= ndev) { g_create_error = "mer_context_create: device id out of range"; return 1; }
    mer_context *ctx = new mer_context();
    ctx->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipGetDeviceProperties(&ctx->prop, device_id) != hipSuccess) {
        g_create_error = "mer_context_create: hipSetDevice failed"; delete ctx; return 1;
    }
    const size_t counter_bytes = sizeof(unsigned long long) * (MER_C_COUNT * MER_COUNTER_REPLICAS + 8);
    bool ok = !ctx->counters.alloc(ctx, counter_bytes) && hipMemset(ctx->counters.p, 0, counter_bytes) == hipSuccess &&
              hipEventCreate(&ctx->ev0) == hipSuccess && hipEventCreate(&ctx->ev1) == hipSuccess;
#ifdef MER_BOUNDS_CHECK
    ok = ok && !ctx->chk_buf.alloc(ctx, 4 * sizeof(unsigned long long)) && hipMemset(ctx->chk_buf.p, 0, 4 * sizeof(unsigned long long)) == hipSuccess;
    ctx->chk = ctx->chk_buf.as<unsigned long long>();
#endif
    if (!ok) { g_create_error = "mer_context_create: device allocation failed"; mer_context_destroy(ctx); return 1; }
    // MER_OPTIONS="name=value,name=value": initial option values for A/B scripts (read once, here; mer_context_set_option afterwards)
    if (const char *e = getenv("MER_OPTIONS")) {
        std::string all(e); size_t pos = 0;
        while (pos < all.size()) {
            size_t end = all.find(',', pos); if (end == std::string::npos) end = all.size();
            const std::string kv = all.substr(pos, end - pos); const size_t eq = kv.find('=');
            if (eq != std::string::npos && mer_context_set_option(ctx, kv.substr(0, eq).c_str(), atoll(kv.c_str() + eq + 1)) != 0) {
                g_create_error = "mer_context_create: MER_OPTIONS: " + ctx->error; mer_context_destroy(ctx); return 1;
            }
            pos = end + 1;
        }
    }
    *out = ctx;
    return 0;
}

// every option: its name, its field and its range (ANY: every value).  The one table behind mer_context_set_option, mer_context_get_option and
// MER_OPTIONS; p = nullptr, with the context's message set, for a name it does not hold.
struct OptionEntry { const char *name; int64_t *p; int64_t min, max; };
static OptionEntry option_slot(mer_context *ctx, const char *name) {
    Options &o = ctx->opt;
    const int64_t ANY = INT64_MAX;
    const OptionEntry table[] = {
        {"pipes", &o.pipes, 1, MER_MAX_PIPES}, {"nslots", &o.nslots, 0, (int64_t) 1 << 28}, {"ksteps", &o.ksteps, 1, 1 << 20}, {"mq_sort", &o.mq_sort, -1, 1},
        {"connect_launches", &o.connect_launches, 1, 64}, {"adaptive_k", &o.adaptive_k, 0, 2}, {"pass_events", &o.pass_events, -ANY - 1, ANY},
        {"buffer_loads", &o.buffer_loads, -ANY - 1, ANY}, {"gen_all", &o.gen_all, -ANY - 1, ANY}, {"prefilter", &o.prefilter, 0, 5},
        {"verbose", &o.verbose, -ANY - 1, ANY}, {"debug_pixel", &o.debug_pixel, -1, ((int64_t) 1 << 31) - 1}, {"lds_bricks", &o.lds_bricks, -ANY - 1, ANY},
        {"march_lds_kb", &o.march_lds_kb, 0, 64},          // dynamic LDS above 64 KiB would need hipFuncSetAttribute
        {"tile_deal", &o.tile_deal, 0, 1}, {"small_render_slots", &o.small_render_slots, 0, 1}, {"inline_walks", &o.inline_walks, 0, 1},
        {"spawn_walks", &o.spawn_walks, 0, 1}, {"grid_fit", &o.grid_fit, 0, 1}, {"check_every", &o.check_every, 1, 64},
        {"march_sort", &o.march_sort, 0, 4}, {"march_sort_major", &o.march_sort_major, 0, 1}};
    for (const auto &t : table) if (std::strcmp(t.name, name) == 0) return t;
    ctx->error = std::string("unknown option '") + name + "'";
    return OptionEntry{name, nullptr, 0, 0};
}
int mer_context_set_option(mer_context *ctx, const char *name, int64_t value) {
    MER_USE_DEVICE(ctx);
    if (!ctx || !name) return 1;
    const OptionEntry t = option_slot(ctx, name);
    if (!t.p) return 1;
    // nslots: 0 = default, otherwise at least one block per pipeline (a smaller value would launch empty grids)
    const bool nslots_too_few = t.p == &ctx->opt.nslots && value > 0 && value < MER_BLOCK * MER_MAX_PIPES;
    if (value < t.min || value > t.max || nslots_too_few) return fail(ctx, std::string("option '") + name + "': value out of range");
    *t.p = value;
    return 0;
}
int mer_context_get_option(mer_context *ctx, const char *name, int64_t *value) {
    MER_USE_DEVICE(ctx);
    if (!ctx || !name || !value) return 1;
    const OptionEntry t = option_slot(ctx, name);
    if (!t.p) return 1;
    *value = *t.p;
    return 0;
}
int mer_debug_bounds(mer_context *ctx, int32_t *enabled, uint64_t out[4]) {
    MER_USE_DEVICE(ctx);
    if (!ctx || !enabled || !out) return 1;
    out[0] = out[1] = out[2] = out[3] = 0;
    *enabled = ctx->chk != nullptr;
    if (ctx->chk) {
        HIP_CHECK(ctx, hipDeviceSynchronize());
        HIP_CHECK(ctx, hipMemcpy(out, ctx->chk, 4 * sizeof(uint64_t), hipMemcpyDeviceToHost));
        HIP_CHECK(ctx, hipMemset(ctx->chk, 0, 4 * sizeof(uint64_t)));
    }
    return 0;
}

// what is not memory: the device buffers of the context, its pipelines, volumes, envmaps and recorders free themselves with `delete ctx`,
// on the device selected here
void mer_context_destroy(mer_context *ctx) {
    if (!ctx) return;
    (void) hipSetDevice(ctx->device);
    for (Pipe &pp : ctx->pipes) {
        for (hipEvent_t e : pp.readback) if (e) (void) hipEventDestroy(e);
        if (pp.finished) (void) hipEventDestroy(pp.finished);
        for (hipEvent_t e : pp.pass_events) (void) hipEventDestroy(e);
        if (pp.own_stream) (void) hipStreamDestroy(pp.own_stream);
    }
    if (ctx->ev0) (void) hipEventDestroy(ctx->ev0);
    if (ctx->ev1) (void) hipEventDestroy(ctx->ev1);
    delete ctx;
}

const char *mer_last_error(mer_context *ctx) { return ctx ? ctx->error.c_str() : g_create_error.c_str(); }

int mer_context_set_stream(mer_context *ctx, void *hip_stream) { ctx->stream = (hipStream_t) hip_stream; return 0; }

int mer_device_info(mer_context *ctx, char *name, int32_t name_len, int32_t *cu_count, int64_t *hbm_bytes) {
    MER_USE_DEVICE(ctx);
    if (name && name_len > 0) { std::strncpy(name, ctx->prop.name, name_len - 1); name[name_len - 1] = 0; }
    if (cu_count) *cu_count = ctx->prop.multiProcessorCount;
    if (hbm_bytes) *hbm_bytes = (int64_t) ctx->prop.totalGlobalMem;
    return 0;
}

static int volume_finish(mer_context *ctx, Volume &v, int32_t layout, mer_volume *out) {
    if (layout == MER_LAYOUT_AUTO) {
        const int64_t nodes = (int64_t) v.desc.res[0] * v.desc.res[1] * v.desc.res[2];
        bool affine = false, zero = true;          // a toWorld transform: the record layouts carry none
        for (int i = 0; i < 12; i++) { const float w = v.desc.world_to_volume[i]; zero = zero && w == 0; affine = affine || w != ((i % 5 == 0) ? 1.0f : 0.0f); }
        layout = (v.desc.channels != 1 || v.desc.dtype != MER_VOL_F32 || (affine && !zero)) ? MER_LAYOUT_DENSE : (nodes <= ((int64_t) 1 << 28) ? MER_LAYOUT_BRICK27 : MER_LAYOUT_CELL8);
    }
    if (layout == MER_LAYOUT_CELL8) {
        if (v.desc.channels != 1 || v.desc.dtype != MER_VOL_F32) return fail(ctx, "CELL8 layout needs a 1-channel float32 grid");
        const size_t ncell = (size_t) (v.desc.res[0] - 1) * (v.desc.res[1] - 1) * (v.desc.res[2] - 1);
        if (v.cell8.alloc(ctx, ncell * 8 * sizeof(float))) return 1;
        hipLaunchKernelGGL(relayout_cell8_kernel, dim3(4096), dim3(256), 0, ctx->stream, v.dense.as<const float>(), v.cell8.as<float>(),
                           v.desc.res[0], v.desc.res[1], v.desc.res[2]);
        HIP_CHECK(ctx, hipGetLastError());
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    } else if (layout == MER_LAYOUT_BRICK27 || layout == MER_LAYOUT_BRICK125) {
        if (v.desc.channels != 1 || v.desc.dtype != MER_VOL_F32) return fail(ctx, "the BRICK layouts need a 1-channel float32 grid");
        const int bshift = layout == MER_LAYOUT_BRICK125 ? 2 : 1, bc = 1 << bshift, recw = layout == MER_LAYOUT_BRICK125 ? 128 : 32;
        for (int i = 0; i < 3; i++) if (v.desc.res[i] < 2) return fail(ctx, "the BRICK layouts need at least 2 nodes per axis");
        const int nbx = (v.desc.res[0] - 2) / bc + 1, nby = (v.desc.res[1] - 2) / bc + 1, nbz = (v.desc.res[2] - 2) / bc + 1;
        if (v.cell8.alloc(ctx, (size_t) nbx * nby * nbz * recw * sizeof(float))) return 1;
        hipLaunchKernelGGL(relayout_brick_kernel, dim3(4096), dim3(256), 0, ctx->stream, v.dense.as<const float>(), v.cell8.as<float>(),
                           v.desc.res[0], v.desc.res[1], v.desc.res[2], nbx, nby, nbz, bshift, recw);
        HIP_CHECK(ctx, hipGetLastError());
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    } else if (layout != MER_LAYOUT_DENSE) return fail(ctx, "unknown volume layout");
    v.layout = layout;
    const int h = ctx->next_handle++;
    ctx->volumes[h] = std::move(v);
    *out = h;
    return 0;
}

static int check_desc(mer_context *ctx, const mer_grid_desc *d) {
    // GridDataSource::loadFromFile checks (src/volume/gridvolume.cpp:243-268)
    if (d->dtype != MER_VOL_F32 && d->dtype != MER_VOL_U8) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "Encountered a volume data file of unknown type (type=%i, channels=%i)!", d->dtype, d->channels);
        return fail(ctx, buf);
    }
    if (d->channels != 1 && d->channels != 3) {
        char buf[160];
        std::snprintf(buf, sizeof(buf), "Encountered an unsupported volume data file (%i channels, only 1 and 3 are supported)", d->channels);
        return fail(ctx, buf);
    }
    for (int i = 0; i < 3; i++) {
        if (d->res[i] < 2) return fail(ctx, "volume resolution must be at least 2 along every axis");
        if (!(d->aabb_min[i] < d->aabb_max[i])) return fail(ctx, "volume bounding box is empty");
    }
    if ((int64_t) d->res[0] * d->res[1] * d->res[2] > (int64_t) 1 << 31) return fail(ctx, "volume too large for the int32 index contract");
    {   // world_to_volume: all zeros (identity) or an invertible affine map
        const float *W = d->world_to_volume; bool zero = true, finite = true;
        for (int i = 0; i < 12; i++) { zero = zero && W[i] == 0.0f; finite = finite && std::isfinite(W[i]); }
        double M[3][3];
        linear3(W, M);
        if (!zero && (!finite || !(std::fabs(det3(M)) > 1e-12))) return fail(ctx, "volume: the toWorld transform is not invertible");
    }
    return 0;
}

// one body for both sources of the dense data: host memory, or device memory of this context's GPU
static int volume_upload(mer_context *ctx, const mer_grid_desc *desc, const void *data, bool from_device, int32_t layout, mer_volume *out) {
    MER_USE_DEVICE(ctx);
    if (!ctx || !desc || !data || !out) return 1;
    if (check_desc(ctx, desc)) return 1;
    HIP_CHECK(ctx, hipSetDevice(ctx->device));
    Volume v; v.desc = *desc;
    const size_t n = (size_t) desc->res[0] * desc->res[1] * desc->res[2] * desc->channels;
    v.bytes_dense = n * (desc->dtype == MER_VOL_F32 ? 4 : 1);
    if (v.dense.alloc(ctx, v.bytes_dense)) return 1;
    if (from_device) {
        HIP_CHECK(ctx, hipMemcpyAsync(v.dense.p, data, v.bytes_dense, hipMemcpyDeviceToDevice, ctx->stream));
        HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        HIP_CHECK(ctx, hipMemcpy(v.dense.p, data, v.bytes_dense, hipMemcpyHostToDevice));
    }
    return volume_finish(ctx, v, layout, out);
}
int mer_volume_upload(mer_context *ctx, const mer_grid_desc *desc, const void *host_data, int32_t layout, mer_volume *out) {
    return volume_upload(ctx, desc, host_data, false, layout, out);
}
int mer_volume_upload_dev(mer_context *ctx, const mer_grid_desc *desc, const void *data_dev, int32_t layout, mer_volume *out) {
    return volume_upload(ctx, desc, data_dev, true, layout, out);
}

int mer_sdf_from_mesh(mer_context *ctx, const mer_grid_desc *desc, const float *vertices, int64_t n_vertices, const int32_t *triangles, int64_t n_triangles,
                      int32_t max_triangles_per_launch, int32_t layout, float *winding_host, mer_volume *out) {
    MER_USE_DEVICE(ctx);
    if (!ctx || !desc || !out) return 1;
    // everything is refused here, before anything reaches the device
    if (desc->channels != 1 || desc->dtype != MER_VOL_F32) return fail(ctx, "mer_sdf_from_mesh: the grid must have channels = 1 and dtype = MER_VOL_F32");
    for (int a = 0; a < 3; a++) if (desc->res[a] < 2) return fail(ctx, "mer_sdf_from_mesh: the grid needs at least 2 nodes along every axis");
    if ((int64_t) desc->res[0] * desc->res[1] * desc->res[2] > (int64_t) 1 << 31) return fail(ctx, "mer_sdf_from_mesh: more than 2^31 nodes");
    for (int a = 0; a < 3; a++)
        if (!std::isfinite(desc->aabb_min[a]) || !std::isfinite(desc->aabb_max[a]) || !(desc->aabb_min[a] < desc->aabb_max[a]))
            return fail(ctx, "mer_sdf_from_mesh: the box is empty or not finite");
    for (int i = 0; i < 12; i++) if (desc->world_to_volume[i] != 0.0f) return fail(ctx, "mer_sdf_from_mesh: a non-zero world_to_volume is not supported");
    if (max_triangles_per_launch < 0) return fail(ctx, "mer_sdf_from_mesh: max_triangles_per_launch must not be negative");
    if (n_triangles < 1 || n_triangles > ((int64_t) 1 << 22) || !triangles) return fail(ctx, "mer_sdf_from_mesh: n_triangles must be in [1, 2^22]");
    if (n_vertices < 1 || !vertices) return fail(ctx, "mer_sdf_from_mesh: the mesh has no vertices");
    for (int64_t i = 0; i < 3 * n_triangles; i++)
        if (triangles[i] < 0 || triangles[i] >= n_vertices) return fail(ctx, "mer_sdf_from_mesh: triangle index out of range");
    for (int64_t i = 0; i < 3 * n_vertices; i++) if (!std::isfinite(vertices[i])) return fail(ctx, "mer_sdf_from_mesh: a vertex is not finite");
    // drop triangles with a repeated index or an exactly zero cross product; 12 floats per kept triangle
    std::vector<float> tri12;
    tri12.reserve((size_t) n_triangles * 12);
    for (int64_t t = 0; t < n_triangles; t++) {
        const int32_t i0 = triangles[3 * t], i1 = triangles[3 * t + 1], i2 = triangles[3 * t + 2];
        if (i0 == i1 || i1 == i2 || i0 == i2) continue;
        const float *a = vertices + 3 * (size_t) i0, *b = vertices + 3 * (size_t) i1, *c = vertices + 3 * (size_t) i2;
        const float e1[3] = {b[0] - a[0], b[1] - a[1], b[2] - a[2]}, e2[3] = {c[0] - a[0], c[1] - a[1], c[2] - a[2]};
        const float nx = e1[1] * e2[2] - e1[2] * e2[1], ny = e1[2] * e2[0] - e1[0] * e2[2], nz = e1[0] * e2[1] - e1[1] * e2[0];
        if (nx == 0.0f && ny == 0.0f && nz == 0.0f) continue;
        for (const float *v : {a, b, c}) { tri12.push_back(v[0]); tri12.push_back(v[1]); tri12.push_back(v[2]); tri12.push_back(0.0f); }
    }
    const int64_t kept = (int64_t) (tri12.size() / 12);
    if (kept == 0) return fail(ctx, "mer_sdf_from_mesh: no triangle left after dropping the degenerate ones");
    DeviceBuffer sdf, winding;
    if (sdf_build(ctx, desc, tri12.data(), kept, max_triangles_per_launch, sdf, winding)) return 1;
    const size_t nodes = (size_t) desc->res[0] * desc->res[1] * desc->res[2];
    if (winding_host && hipMemcpy(winding_host, winding.p, nodes * 4, hipMemcpyDeviceToHost) != hipSuccess) return fail(ctx, "mer_sdf_from_mesh: copy of the winding numbers failed");
    return volume_upload(ctx, desc, sdf.p, true, layout, out);         // the path of mer_volume_upload_dev
}

int mer_volume_download(mer_context *ctx, mer_volume h, float *data_host) {
    MER_USE_DEVICE(ctx);
    if (!ctx || !data_host) return 1;
    if (ctx->envmaps.count(h)) return fail(ctx, "mer_volume_download: an envmap handle has no grid payload");
    auto it = ctx->volumes.find(h);
    if (it == ctx->volumes.end()) return fail(ctx, "invalid volume handle");
    const Volume &v = it->second;
    if (v.desc.channels != 1 || v.desc.dtype != MER_VOL_F32) return fail(ctx, "mer_volume_download: only a 1-channel float32 volume can be downloaded");
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    HIP_CHECK(ctx, hipMemcpy(data_host, v.dense.p, v.bytes_dense, hipMemcpyDeviceToHost));
    return 0;
}

int mer_volume_build_spline(mer_context *ctx, mer_volume h) {
    MER_USE_DEVICE(ctx);
    auto it = ctx->volumes.find(h);
    if (it == ctx->volumes.end()) return fail(ctx, "invalid volume handle");
    Volume &v = it->second;
    if (v.desc.channels != 1 || v.desc.dtype != MER_VOL_F32) return fail(ctx, "splinevolume needs a 1-channel float32 grid");
    if (v.coeff) return 0;
    const int nx = v.desc.res[0], ny = v.desc.res[1], nz = v.desc.res[2];
    const size_t n = (size_t) nx * ny * nz;
    DeviceBuffer abuf, bbuf, tbuf;
    if (abuf.alloc(ctx, n * 4) || bbuf.alloc(ctx, n * 4)) return 1;
    float *a = abuf.as<float>(), *b = bbuf.as<float>(), *t = nullptr;
    const float *dense = v.dense.as<const float>();
    // along y (lines indexed by x and z), then x (by y and z), then z (by x and y): basisspline.h:868-887
    const int64_t form = ctx->opt.prefilter;
    const bool seq = form == 1 || std::min(nx, std::min(ny, nz)) < 16;
    if (seq) {                 // one thread per line (reference order of operations; tiny grids)
        hipLaunchKernelGGL(bspline_pass_kernel, dim3(nblocks((int64_t) nx * nz)), dim3(256), 0, ctx->stream,
                           dense, a, nx, nz, (int64_t) 1, (int64_t) nx * ny, (int64_t) nx, ny);
        hipLaunchKernelGGL(bspline_pass_kernel, dim3(nblocks((int64_t) ny * nz)), dim3(256), 0, ctx->stream,
                           (const float *) a, b, ny, nz, (int64_t) nx, (int64_t) nx * ny, (int64_t) 1, nx);
        hipLaunchKernelGGL(bspline_pass_kernel, dim3(nblocks((int64_t) nx * ny)), dim3(256), 0, ctx->stream,
                           (const float *) b, a, nx, ny, (int64_t) 1, (int64_t) nx, (int64_t) nx * ny, nz);
    } else {
        if (form == 2 || form == 3) { if (tbuf.alloc(ctx, n * 4)) return 1; t = tbuf.as<float>(); }
        auto pass = [&](const float *src, float *dst, int na, int nb, int64_t sa, int64_t sb, int64_t sl, int size) {
            const int64_t threads = (int64_t) na * nb * ((size + MER_PF_SEG - 1) / MER_PF_SEG);
            hipLaunchKernelGGL(bspline_causal_kernel, dim3(nblocks(threads)), dim3(256), 0, ctx->stream, src, t, na, nb, sa, sb, sl, size);
            hipLaunchKernelGGL(bspline_anticausal_kernel, dim3(nblocks(threads)), dim3(256), 0, ctx->stream, (const float *) t, dst, na, nb, sa, sb, sl, size);
        };
        auto win = [&](const float *src, float *dst, int na, int nb, int64_t sb, int64_t sl, int size) {     // fused sweeps, unit stride in a
            const int nseg = (size + MER_PF_SEG - 1) / MER_PF_SEG;
            // interior segments (window inside the line): wave-uniform addressing, no per-sample conditions (bspline_win2_kernel); border segments: generic kernel
            int s_lo = 0, s_hi = nseg;
            if (form != 5 && nb <= 65535 && sl * 4 * (int64_t) MER_PFX_W < ((int64_t) 1 << 31)) {
                while (s_lo < nseg && !(s_lo * MER_PF_SEG - MER_PF_WARM > 0)) s_lo++;
                s_hi = s_lo;
                while (s_hi < nseg && s_hi * MER_PF_SEG - MER_PF_WARM + MER_PFX_W < size) s_hi++;
            } else s_lo = nseg;
            if (s_hi > s_lo)
                hipLaunchKernelGGL(bspline_win2_kernel, dim3((unsigned) ((na + 255) / 256), (unsigned) (s_hi - s_lo), (unsigned) nb), dim3(256), 0, ctx->stream, src, dst, na, sb, sl, size, s_lo);
            else { s_lo = nseg; s_hi = nseg; }
            const int64_t threads = (int64_t) na * nb * (s_lo + (nseg - s_hi));
            if (threads > 0) hipLaunchKernelGGL(bspline_win_kernel, dim3(nblocks(threads)), dim3(256), 0, ctx->stream, src, dst, na, nb, sb, sl, size, s_lo, s_hi);
        };
        const bool two_kernel = form == 2;
        if (two_kernel) pass(dense, a, nx, nz, 1, (int64_t) nx * ny, nx, ny);          // y
        else win(dense, a, nx, nz, (int64_t) nx * ny, nx, ny);
        if (form == 3) pass(a, b, ny, nz, nx, (int64_t) nx * ny, 1, nx);           // x, strided form
        else {                                                                                        // x: lines are contiguous -> LDS tiles
            const int64_t nlines = (int64_t) ny * nz;
            const int ntile = (nx + MER_PFX_COLS - 1) / MER_PFX_COLS;
            int t_lo = ntile, t_hi = ntile;                       // interior segments in registers (n % 4 == 0), border tiles through LDS
            if (nx % 4 == 0 && form != 4) {
                t_lo = 0; while (t_lo < ntile && !(t_lo * MER_PF_SEG - MER_PF_WARM > 0)) t_lo++;
                t_hi = t_lo; while (t_hi < ntile && t_hi * MER_PF_SEG - MER_PF_WARM + MER_PFX_W < nx) t_hi++;
                if (t_hi > t_lo) {
                    const int64_t threads = nlines * (t_hi - t_lo);
                    hipLaunchKernelGGL(bspline_x_reg_kernel, dim3(nblocks(threads)), dim3(256), 0, ctx->stream, (const float *) a, b, nlines, nx, t_lo, t_hi - t_lo);
                } else t_lo = t_hi = ntile;
            }
            if (nx % 4 == 0 && form != 4) {        // border segments: the guarded register form
                const int64_t threads = nlines * (t_lo + (ntile - t_hi));
                if (threads > 0) hipLaunchKernelGGL(bspline_x_reg_border_kernel, dim3(nblocks(threads)), dim3(256), 0, ctx->stream, (const float *) a, b, nlines, nx, t_lo, t_hi);
            } else {                                // any line length: LDS tiles
                const int64_t blocks = ((nlines + MER_PFX_ROWS - 1) / MER_PFX_ROWS) * (t_lo + (ntile - t_hi));
                if (blocks > 0) hipLaunchKernelGGL(bspline_x_kernel, dim3((unsigned) blocks), dim3(256), 0, ctx->stream, (const float *) a, b, nlines, nx, t_lo, t_hi);
            }
        }
        if (two_kernel) pass(b, a, nx, ny, 1, nx, (int64_t) nx * ny, nz);                                // z
        else win(b, a, nx, ny, nx, (int64_t) nx * ny, nz);
    }
    HIP_CHECK(ctx, hipGetLastError());
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    v.coeff = std::move(abuf);
    return 0;
}

int mer_volume_download_spline(mer_context *ctx, mer_volume h, float *coeff_host) {
    MER_USE_DEVICE(ctx);
    auto it = ctx->volumes.find(h);
    if (it == ctx->volumes.end() || !it->second.coeff) return fail(ctx, "volume has no spline coefficients");
    const size_t n = (size_t) it->second.desc.res[0] * it->second.desc.res[1] * it->second.desc.res[2];
    HIP_CHECK(ctx, hipMemcpy(coeff_host, it->second.coeff.p, n * 4, hipMemcpyDeviceToHost));
    return 0;
}

int mer_volume_destroy(mer_context *ctx, mer_volume h) {
    MER_USE_DEVICE(ctx);
    auto ie = ctx->envmaps.find(h);
    if (ie != ctx->envmaps.end()) { ctx->envmaps.erase(ie); return 0; }             // an envmap (mer_envmap_upload)
    auto it = ctx->volumes.find(h);
    if (it == ctx->volumes.end()) return fail(ctx, "invalid volume handle");
    ctx->volumes.erase(it);
    return 0;
}

// IEEE binary16, round to nearest even (OpenEXR's half(float), which the reference's SpectrumHalf texels use; overflow -> inf)
static uint16_t float_to_half(float f) { const _Float16 h = (_Float16) f; uint16_t b; std::memcpy(&b, &h, 2); return b; }
static float half_to_float(uint16_t b) { _Float16 h; std::memcpy(&h, &b, 2); return (float) h; }

// EnvironmentMap::configure() (src/emitters/envmap.cpp:260-320) on the half-rounded texels: Float = float accumulations in x / y order, the
// tables stored as float, sin of the double expression, the normalisation formed in double and rounded (the library is built with
// -ffp-contract=off: each product is rounded as the reference's scalar code rounds it).
static int envmap_tables(mer_context *ctx, int W, int H, const std::vector<uint16_t> &tex, std::vector<float> &cols, std::vector<float> &rows,
                         std::vector<float> &weights, float &norm) {
    cols.assign((size_t) (W + 1) * H, 0.0f); rows.assign((size_t) H + 1, 0.0f); weights.assign((size_t) H, 0.0f);
    size_t colPos = 0, rowPos = 0;
    float rowSum = 0.0f;
    rows[rowPos++] = 0;
    for (int y = 0; y < H; ++y) {
        float colSum = 0;
        cols[colPos++] = 0;
        for (int x = 0; x < W; ++x) {
            const uint16_t *t = &tex[((size_t) y * W + x) * 4];
            const float lum = half_to_float(t[0]) * 0.212671f + half_to_float(t[1]) * 0.715160f + half_to_float(t[2]) * 0.072169f;
            colSum += lum;
            cols[colPos++] = colSum;
        }
        const float normalization = 1.0f / colSum;
        for (int x = 1; x < W; ++x) cols[colPos - x - 1] *= normalization;
        cols[colPos - 1] = 1.0f;
        const float weight = (float) std::sin((double) (y + 0.5f) * M_PI / H);
        weights[y] = weight;
        rowSum += colSum * weight;
        rows[rowPos++] = rowSum;
    }
    const float normalization = 1.0f / rowSum;
    for (int y = 1; y < H; ++y) rows[rowPos - y - 1] *= normalization;
    rows[rowPos - 1] = 1.0f;
    if (rowSum == 0) return fail(ctx, "The environment map is completely black -- this is not allowed.");
    if (!std::isfinite(rowSum)) return fail(ctx, "The environment map contains an invalid floating point value (nan/inf) -- giving up.");
    norm = (float) (1.0f / ((double) rowSum * (2 * M_PI / W) * (M_PI / H)));
    return 0;
}

int mer_envmap_upload(mer_context *ctx, int32_t width, int32_t height, const float *rgb_host, mer_volume *out) {
    MER_USE_DEVICE(ctx);
    if (!out) return fail(ctx, "mer_envmap_upload: no output handle");
    if (width < 1 || height < 1 || !rgb_host) return fail(ctx, "mer_envmap_upload: the image must have at least one pixel");
    if (std::max(width, height) > 0xFFFF) return fail(ctx, "Environment maps images must be smaller than 65536 pixels in width and height");
    const size_t npix = (size_t) width * height;
    std::vector<uint16_t> tex(npix * 4, 0);
    for (size_t i = 0; i < npix; ++i)
        for (int c = 0; c < 3; c++) tex[4 * i + c] = float_to_half(rgb_host[3 * i + c]);
    EnvMap m; m.w = width; m.h = height;
    std::vector<float> cols, rows, weights;
    if (envmap_tables(ctx, width, height, tex, cols, rows, weights, m.norm)) return 1;
    auto up16 = [](size_t b) { return (b + 15) & ~(size_t) 15; };
    m.off_cols = up16(npix * 8); m.off_rows = up16(m.off_cols + cols.size() * 4); m.off_weights = up16(m.off_rows + rows.size() * 4);
    const size_t bytes = m.off_weights + weights.size() * 4;
    std::vector<unsigned char> h(bytes, 0);
    std::memcpy(h.data(), tex.data(), npix * 8);
    std::memcpy(h.data() + m.off_cols, cols.data(), cols.size() * 4);
    std::memcpy(h.data() + m.off_rows, rows.data(), rows.size() * 4);
    std::memcpy(h.data() + m.off_weights, weights.data(), weights.size() * 4);
    if (m.dev.alloc(ctx, bytes)) return 1;
    if (hipMemcpy(m.dev.p, h.data(), bytes, hipMemcpyHostToDevice) != hipSuccess) return fail(ctx, "mer_envmap_upload: copy to the device failed");
    const int hd = ctx->next_handle++;
    ctx->envmaps[hd] = std::move(m);
    *out = hd;
    return 0;
}

int mer_film_channels(mer_context *ctx, const mer_scene_desc *scene, int32_t *channels) {
    MER_USE_DEVICE(ctx);
    int frames;
    if (!scene || !channels) return 1;
    if (film_frames(ctx, scene, frames)) return 1;
    *channels = frames * 3 + 2;
    return 0;
}
int mer_film_alloc_n(mer_context *ctx, int32_t width, int32_t height, int32_t channels, float **film_dev) {
    MER_USE_DEVICE(ctx);
    DeviceBuffer film;               // the caller's from here on (mer_film_free)
    if (film.alloc(ctx, (size_t) width * height * channels * sizeof(float))) return 1;
    HIP_CHECK(ctx, hipMemsetAsync(film.p, 0, (size_t) width * height * channels * sizeof(float), ctx->stream));
    *film_dev = (float *) film.release();
    return 0;
}
int mer_film_zero_n(mer_context *ctx, float *film_dev, int32_t width, int32_t height, int32_t channels) {
    MER_USE_DEVICE(ctx);
    HIP_CHECK(ctx, hipMemsetAsync(film_dev, 0, (size_t) width * height * channels * sizeof(float), ctx->stream));
    return 0;
}
int mer_film_download_n(mer_context *ctx, const float *film_dev, int32_t width, int32_t height, int32_t channels, float *film_host) {
    MER_USE_DEVICE(ctx);
    HIP_CHECK(ctx, hipMemcpyAsync(film_host, film_dev, (size_t) width * height * channels * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
int mer_film_alloc(mer_context *ctx, int32_t width, int32_t height, float **film_dev) { return mer_film_alloc_n(ctx, width, height, 5, film_dev); }
int mer_film_zero(mer_context *ctx, float *film_dev, int32_t width, int32_t height) { return mer_film_zero_n(ctx, film_dev, width, height, 5); }
int mer_film_download(mer_context *ctx, const float *film_dev, int32_t width, int32_t height, float *film_host) {
    MER_USE_DEVICE(ctx);
    return mer_film_download_n(ctx, film_dev, width, height, 5, film_host);
}
int mer_film_free(mer_context *ctx, float *film_dev) { return DeviceBuffer::free_raw(ctx, film_dev); }
int mer_device_free(mer_context *ctx, void *p) { return DeviceBuffer::free_raw(ctx, p); }

int mer_render(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, float *film_dev) {
    MER_USE_DEVICE(ctx);
    if (!ctx || !scene || !film_dev) return 1;
    int32_t ch = 5;
    if (mer_film_channels(ctx, scene, &ch)) return 1;
    if (scene->integrator == MER_INTEGRATOR_PTRACER) return launch_ptracer(ctx, scene, shard, seed, film_dev, (uint64_t) scene->width * scene->height * (uint64_t) ch);
    return launch_render(ctx, scene, shard, seed, film_dev, nullptr, (uint64_t) scene->width * scene->height * (uint64_t) ch, 0);
}

int mer_render_paths(mer_context *ctx, const mer_scene_desc *scene, int32_t sample_index, uint64_t seed, float *out_rgb) {
    MER_USE_DEVICE(ctx);
    if (!ctx || !scene || !out_rgb) return 1;
    if (scene->integrator == MER_INTEGRATOR_PTRACER) return fail(ctx, "mer_render_paths: per-path radiance is a camera-path quantity (integrator = volpath); a light path splats onto many pixels");
    const size_t n = (size_t) scene->width * scene->height * 3;
    DeviceBuffer buf;
    if (buf.alloc(ctx, n * 4)) return 1;
    HIP_CHECK(ctx, hipMemsetAsync(buf.p, 0, n * 4, ctx->stream));
    mer_shard sh = {sample_index, 1, 1, 0, 1};
    if (launch_render(ctx, scene, &sh, seed, buf.as<float>(), buf.as<float>(), n, n)) return 1;
    return buf.download(ctx, out_rgb, n * 4);
}

int mer_synchronize(mer_context *ctx) { HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream)); return 0; }

int mer_last_kernel_ms(mer_context *ctx, float *ms) {
    MER_USE_DEVICE(ctx);
    if (!ctx->timed) return fail(ctx, "no render has been launched");
    HIP_CHECK(ctx, hipEventSynchronize(ctx->ev1));
    HIP_CHECK(ctx, hipEventElapsedTime(ms, ctx->ev0, ctx->ev1));
    return 0;
}

int mer_last_render_stats(mer_context *ctx, int32_t *passes, float *march_ms, float *event_ms) {
    MER_USE_DEVICE(ctx);
    if (!ctx->timed) return fail(ctx, "no render has been launched");
    if (passes) *passes = ctx->last_passes;
    if (march_ms) *march_ms = ctx->last_march_ms;
    if (event_ms) *event_ms = ctx->last_event_ms;
    return 0;
}

int mer_counters_read(mer_context *ctx, uint64_t out[MER_C_COUNT]) {
    MER_USE_DEVICE(ctx);
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    std::vector<uint64_t> all((size_t) MER_C_COUNT * MER_COUNTER_REPLICAS);
    HIP_CHECK(ctx, hipMemcpy(all.data(), ctx->counters.p, sizeof(uint64_t) * all.size(), hipMemcpyDeviceToHost));
    for (int k = 0; k < MER_C_COUNT; k++) {
        out[k] = 0;
        for (int r = 0; r < MER_COUNTER_REPLICAS; r++) out[k] += all[(size_t) r * MER_C_COUNT + k];
    }
    return 0;
}
int mer_counters_reset(mer_context *ctx) {
    MER_USE_DEVICE(ctx);
    HIP_CHECK(ctx, hipMemsetAsync(ctx->counters.p, 0, sizeof(uint64_t) * MER_C_COUNT * MER_COUNTER_REPLICAS, ctx->stream));
    return 0;
}

// ---- leaf entry points ------------------------------------------------------------------------------
int mer_lookup_trilinear(mer_context *ctx, mer_volume h, const float *pts, int64_t n, float *out_val, int32_t *out_idx) {
    MER_USE_DEVICE(ctx);
    auto it = ctx->volumes.find(h);
    if (it == ctx->volumes.end()) return fail(ctx, "invalid volume handle");
    if (it->second.desc.channels != 1) return fail(ctx, "lookupFloat(): volume does not support float lookups");
    DGrid g; fill_dgrid(ctx, it->second, g);
    DeviceBuffer dp, dv, di;
    if (dp.upload(ctx, pts, n * 12) || dv.alloc(ctx, n * 4) || di.alloc(ctx, n * 16)) return 1;
    hipLaunchKernelGGL(lookup_trilinear_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, g, dp.as<float>(), n, dv.as<float>(),
                       out_idx ? di.as<int32_t>() : (int32_t *) nullptr);
    HIP_CHECK(ctx, hipGetLastError());
    if (dv.download(ctx, out_val, n * 4)) return 1;
    if (out_idx && di.download(ctx, out_idx, n * 16)) return 1;
    return 0;
}
int mer_lookup_trilinear_rgb(mer_context *ctx, mer_volume h, const float *pts, int64_t n, float *out_rgb) {
    MER_USE_DEVICE(ctx);
    auto it = ctx->volumes.find(h);
    if (it == ctx->volumes.end()) return fail(ctx, "invalid volume handle");
    if (it->second.desc.channels != 3) return fail(ctx, "lookupSpectrum(): volume does not support spectrum lookups");
    DGrid g; fill_dgrid(ctx, it->second, g, false);
    DeviceBuffer dp, dv;
    if (dp.upload(ctx, pts, n * 12) || dv.alloc(ctx, n * 12)) return 1;
    hipLaunchKernelGGL(lookup_rgb_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, g, dp.as<float>(), n, dv.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return dv.download(ctx, out_rgb, n * 12);
}
int mer_rif_value_grad(mer_context *ctx, mer_volume h, int32_t interp, const float *pts, int64_t n, float *out_val, float *out_grad) {
    MER_USE_DEVICE(ctx);
    auto it = ctx->volumes.find(h);
    if (it == ctx->volumes.end()) return fail(ctx, "invalid volume handle");
    if (it->second.desc.channels != 1 || it->second.desc.dtype != MER_VOL_F32) return fail(ctx, "value(): not implemented for this volume type"); // volume.cpp:57-80
    if (interp != MER_RIF_TRILINEAR && interp != MER_RIF_BSPLINE3) return fail(ctx, "unknown rif_interp");
    if (interp == MER_RIF_BSPLINE3 && !it->second.coeff) return fail(ctx, "volume has no spline coefficients");
    DGrid g; fill_dgrid(ctx, it->second, g);
    DeviceBuffer dp, dv, dg;
    if (dp.upload(ctx, pts, n * 12) || dv.alloc(ctx, n * 4) || dg.alloc(ctx, n * 12)) return 1;
    hipLaunchKernelGGL(rif_value_grad_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, g, interp, dp.as<float>(), n, dv.as<float>(), dg.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    if (dv.download(ctx, out_val, n * 4)) return 1;
    return dg.download(ctx, out_grad, n * 12);
}

int mer_acoustic_value_grad(mer_context *ctx, const mer_scene_desc *scene, const float *pts, int64_t n, float *out_val, float *out_grad) {
    MER_USE_DEVICE(ctx);
    if (scene->rif_mode != MER_RIF_ACOUSTIC) return fail(ctx, "mer_acoustic_value_grad needs rif_mode = acoustic");
    Params P;
    mer_scene_desc sc = *scene; sc.sigma_mode = MER_SIGMA_HOMOGENEOUS; sc.albedo_mode = MER_ALBEDO_CONST;
    if (make_params(ctx, &sc, P)) return 1;
    DeviceBuffer dp, dv, dg;
    if (dp.upload(ctx, pts, n * 12) || dv.alloc(ctx, n * 4) || dg.alloc(ctx, n * 12)) return 1;
    hipLaunchKernelGGL(acoustic_value_grad_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P.rif, dp.as<float>(), n, dv.as<float>(), dg.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    if (dv.download(ctx, out_val, n * 4)) return 1;
    return dg.download(ctx, out_grad, n * 12);
}

int mer_er_trace(mer_context *ctx, const mer_scene_desc *scene, const float *p0, const float *d0, const float *dist, int64_t n,
                 float *out_p, float *out_v, float *out_dist_surf, float *out_opt, int32_t *out_success) {
    MER_USE_DEVICE(ctx);
    Params P;
    if (make_params(ctx, scene, P)) return 1;
    if (scene->rif_mode == MER_RIF_CONST) return fail(ctx, "mer_er_trace needs a RIF volume");
    DeviceBuffer a, b, c, op, ov, od, oo, ok;
    if (a.upload(ctx, p0, n * 12) || b.upload(ctx, d0, n * 12) || c.upload(ctx, dist, n * 4) || op.alloc(ctx, n * 12) || ov.alloc(ctx, n * 12) ||
        od.alloc(ctx, n * 4) || oo.alloc(ctx, n * 4) || ok.alloc(ctx, n * 4)) return 1;
    const int rifk = rif_fetch_kind(ctx, scene);
    match_constant(FetchKinds(), rifk, [&](auto rif) {
        return match_constant(Steppers(), scene->stepper, [&](auto stepper) {
            hipLaunchKernelGGL((er_trace_kernel<decltype(rif)::value, decltype(stepper)::value>), dim3(nblocks(n, 64)), dim3(64), 0, ctx->stream, P, a.as<float>(), b.as<float>(),
                               c.as<float>(), n, op.as<float>(), ov.as<float>(), od.as<float>(), oo.as<float>(), ok.as<int32_t>());
            return true;
        });
    });
    HIP_CHECK(ctx, hipGetLastError());
    if (op.download(ctx, out_p, n * 12) || ov.download(ctx, out_v, n * 12) || od.download(ctx, out_dist_surf, n * 4) || oo.download(ctx, out_opt, n * 4) ||
        ok.download(ctx, out_success, n * 4)) return 1;
    return 0;
}

int mer_connect(mer_context *ctx, const mer_scene_desc *scene, const float *p1, const float *p2, int64_t n, uint64_t seed, float *out) {
    MER_USE_DEVICE(ctx);
    Params P;
    if (make_params(ctx, scene, P, true)) return 1;
    if (scene->rif_mode == MER_RIF_CONST) return fail(ctx, "mer_connect needs a RIF volume");
    if (scene->rif_mode == MER_RIF_ACOUSTIC) return fail(ctx, "mer_connect: the analytic acoustic RIF is connected inside mer_render only");
    P.seed = seed;
    DeviceBuffer a, b, r;
    if (a.upload(ctx, p1, n * 12) || b.upload(ctx, p2, n * 12) || r.alloc(ctx, n * 48)) return 1;
    const int rifk = rif_fetch_kind(ctx, scene);
    bool launched = false;
#define MER_CONNECT_CASE(R, B) if (!launched && rifk == R && (scene->boundary == MER_BOUNDARY_SDF) == (B == 1)) { launched = true;   \
        hipLaunchKernelGGL((connect_kernel<R, B>), dim3(nblocks(n, 64)), dim3(64), 0, ctx->stream, P, a.as<float>(), b.as<float>(), n, r.as<float>()); }
    MER_CONNECT_CASE(MER_RIF_TRILINEAR, 0) MER_CONNECT_CASE(MER_RIF_BSPLINE3, 0) MER_CONNECT_CASE(RIFK_DENSE_BUF, 0) MER_CONNECT_CASE(RIFK_CELL8, 0) MER_CONNECT_CASE(RIFK_CELL8_BUF, 0)
    MER_CONNECT_CASE(RIFK_BRICK27_BUF, 0) MER_CONNECT_CASE(RIFK_BRICK27, 0)
    // signed-distance boundary: the fetch kinds mer_render instantiates for it
    MER_CONNECT_CASE(MER_RIF_TRILINEAR, 1) MER_CONNECT_CASE(RIFK_CELL8_BUF, 1) MER_CONNECT_CASE(MER_RIF_BSPLINE3, 1)
#undef MER_CONNECT_CASE
    if (!launched) {
        // a dense RIF below 4 GiB selects buffer loads; the signed-distance kernels read it with global loads
        if (scene->boundary == MER_BOUNDARY_SDF && rifk == RIFK_DENSE_BUF) {
            hipLaunchKernelGGL((connect_kernel<MER_RIF_TRILINEAR, 1>), dim3(nblocks(n, 64)), dim3(64), 0, ctx->stream, P, a.as<float>(), b.as<float>(), n, r.as<float>());
        } else return fail(ctx, "mer_connect: unsupported RIF layout for this boundary");
    }
    HIP_CHECK(ctx, hipGetLastError());
    return r.download(ctx, out, n * 48);
}

int mer_sample_distance(mer_context *ctx, const mer_scene_desc *scene, const float *o, const float *d, const float *maxt, int64_t n,
                        uint64_t seed, float *rec) {
    MER_USE_DEVICE(ctx);
    Params P;
    if (make_params(ctx, scene, P)) return 1;
    P.seed = seed;
    DeviceBuffer a, b, c, r;
    if (a.upload(ctx, o, n * 12) || b.upload(ctx, d, n * 12) || c.upload(ctx, maxt, n * 4) || r.alloc(ctx, n * 80)) return 1;
    int rc = dispatch_modes(ctx, scene, [&](auto curved, auto rif, auto stepper, auto sigma, auto bnd) -> int {
        hipLaunchKernelGGL((sample_distance_kernel<decltype(curved)::value, decltype(rif)::value, decltype(stepper)::value, decltype(sigma)::value>),
                           dim3(nblocks(n, 64)), dim3(64), 0, ctx->stream, P, a.as<float>(), b.as<float>(), c.as<float>(), n, r.as<float>());
        HIP_CHECK(ctx, hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    return r.download(ctx, rec, n * 80);
}

int mer_eval_transmittance(mer_context *ctx, const mer_scene_desc *scene, const float *o, const float *d, const float *maxt, int64_t n,
                           uint64_t seed, float *out_tr) {
    MER_USE_DEVICE(ctx);
    Params P;
    if (make_params(ctx, scene, P)) return 1;
    P.seed = seed;
    DeviceBuffer a, b, c, r;
    if (a.upload(ctx, o, n * 12) || b.upload(ctx, d, n * 12) || c.upload(ctx, maxt, n * 4) || r.alloc(ctx, n * 12)) return 1;
    int rc = dispatch_modes(ctx, scene, [&](auto curved, auto rif, auto stepper, auto sigma, auto bnd) -> int {
        hipLaunchKernelGGL((eval_transmittance_kernel<decltype(curved)::value, decltype(rif)::value, decltype(stepper)::value, decltype(sigma)::value>),
                           dim3(nblocks(n, 64)), dim3(64), 0, ctx->stream, P, a.as<float>(), b.as<float>(), c.as<float>(), n, r.as<float>());
        HIP_CHECK(ctx, hipGetLastError());
        return 0;
    });
    if (rc) return rc;
    return r.download(ctx, out_tr, n * 12);
}

int mer_phase_sample(mer_context *ctx, int32_t phase, float g, const float *wi, const float *u2, int64_t n, float *wo, float *pdf) {
    MER_USE_DEVICE(ctx);
    if (phase == MER_PHASE_HG && (g >= 1 || g <= -1)) return fail(ctx, "The asymmetry parameter must lie in the interval (-1, 1)!");
    DeviceBuffer a, b, c, e;
    if (a.upload(ctx, wi, n * 12) || b.upload(ctx, u2, n * 8) || c.alloc(ctx, n * 12) || e.alloc(ctx, n * 4)) return 1;
    hipLaunchKernelGGL(phase_sample_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, phase, g, a.as<float>(), b.as<float>(), n, c.as<float>(), e.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    if (c.download(ctx, wo, n * 12)) return 1;
    return e.download(ctx, pdf, n * 4);
}
int mer_phase_eval(mer_context *ctx, int32_t phase, float g, const float *wi, const float *wo, int64_t n, float *val) {
    MER_USE_DEVICE(ctx);
    DeviceBuffer a, b, c;
    if (a.upload(ctx, wi, n * 12) || b.upload(ctx, wo, n * 12) || c.alloc(ctx, n * 4)) return 1;
    hipLaunchKernelGGL(phase_eval_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, phase, g, a.as<float>(), b.as<float>(), n, c.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return c.download(ctx, val, n * 4);
}
int mer_emitter_direct(mer_context *ctx, const mer_scene_desc *scene, int32_t k, const float *ref, int64_t n, float *out) {
    MER_USE_DEVICE(ctx);
    if (scene->n_emitters <= 0 || !scene->emitters) return fail(ctx, "mer_emitter_direct: the scene has no emitter list");
    if (k < 0 || k >= scene->n_emitters) return fail(ctx, "mer_emitter_direct: entry index out of range");
    const int type = scene->emitters[k].type;
    if (type != MER_EMITTER_POINT && type != MER_EMITTER_SPOT) return fail(ctx, "mer_emitter_direct: entry k must be a point or spot emitter");
    int slot = 0;                                   // its slot of the point table: the point / spot entries before it, in list order
    for (int j = 0; j < k; ++j) slot += (scene->emitters[j].type == MER_EMITTER_POINT || scene->emitters[j].type == MER_EMITTER_SPOT) ? 1 : 0;
    Params P;
    if (make_params(ctx, scene, P, true)) return 1;
    if (n <= 0) return 0;
    const float *I = scene->emitters[k].intensity;
    DeviceBuffer a, r;
    if (a.upload(ctx, ref, n * 12) || r.alloc(ctx, n * 32)) return 1;
    hipLaunchKernelGGL(emitter_direct_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P.points, P.has_spot ? &ctx->etab.as<EmitterTable>()->spots[0] : (const DSpot *) nullptr, slot, I[0], I[1], I[2], a.as<float>(), n, r.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return r.download(ctx, out, n * 32);
}
static bool is_area_type(int type) { return type == MER_EMITTER_AREA || type == MER_EMITTER_AREA_DISK || type == MER_EMITTER_AREA_SPHERE; }
int mer_area_direct(mer_context *ctx, const mer_scene_desc *scene, int32_t k, const float *ref, const float *u2, int64_t n, float *out) {
    MER_USE_DEVICE(ctx);
    if (scene->n_emitters <= 0 || !scene->emitters) return fail(ctx, "mer_area_direct: the scene has no emitter list");
    if (k < 0 || k >= scene->n_emitters) return fail(ctx, "mer_area_direct: entry index out of range");
    if (!is_area_type(scene->emitters[k].type)) return fail(ctx, "mer_area_direct: entry k must be an area emitter");
    int slot = 0;                                   // its slot of the area table: the area entries before it, in list order
    for (int j = 0; j < k; ++j) slot += is_area_type(scene->emitters[j].type) ? 1 : 0;
    Params P;
    if (make_params(ctx, scene, P, true)) return 1;
    if (n <= 0) return 0;
    DeviceBuffer a, b, r;
    if (a.upload(ctx, ref, n * 12) || b.upload(ctx, u2, n * 8) || r.alloc(ctx, n * 48)) return 1;
    hipLaunchKernelGGL(area_direct_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P.rects, slot, a.as<float>(), b.as<float>(), n, r.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return r.download(ctx, out, n * 48);
}
int mer_area_hit(mer_context *ctx, const mer_scene_desc *scene, const float *o, const float *d, const float *ref, int64_t n, float *out) {
    MER_USE_DEVICE(ctx);
    if (scene->n_emitters <= 0 || !scene->emitters) return fail(ctx, "mer_area_hit: the scene has no emitter list");
    Params P;
    if (make_params(ctx, scene, P, true)) return 1;
    if (!P.n_rect) return fail(ctx, "mer_area_hit: the scene's emitter list has no area emitter");
    if (n <= 0) return 0;
    int32_t list_index[MER_MAX_EMITTERS] = {0};
    for (int j = 0, slot = 0; j < scene->n_emitters; ++j) if (is_area_type(scene->emitters[j].type)) list_index[slot++] = j;
    DeviceBuffer a, b, c, x, r;
    if (a.upload(ctx, o, n * 12) || b.upload(ctx, d, n * 12) || c.upload(ctx, ref, n * 12) || x.upload(ctx, list_index, sizeof(list_index)) || r.alloc(ctx, n * 32)) return 1;
    hipLaunchKernelGGL(area_hit_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P, x.as<int32_t>(), a.as<float>(), b.as<float>(), c.as<float>(), n, r.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return r.download(ctx, out, n * 32);
}
// the scene's envmap record in device memory (the emitter table's), or NULL
static const DEnvMap *envmap_of(mer_context *ctx, const mer_scene_desc *scene, Params &P, const char *who) {
    if (make_params(ctx, scene, P, true)) return nullptr;
    if (!P.has_envmap) { fail(ctx, std::string(who) + ": the scene's emitter list has no envmap entry"); return nullptr; }
    return &ctx->etab.as<EmitterTable>()->env;
}
int mer_envmap_eval(mer_context *ctx, const mer_scene_desc *scene, const float *dirs, int64_t n, float *out_rgb, float *out_pdf) {
    MER_USE_DEVICE(ctx);
    Params P;
    const DEnvMap *E = envmap_of(ctx, scene, P, "mer_envmap_eval");
    if (!E) return 1;
    if (n <= 0) return 0;
    DeviceBuffer a, v, q;
    if (a.upload(ctx, dirs, n * 12) || v.alloc(ctx, n * 12) || q.alloc(ctx, n * 4)) return 1;
    hipLaunchKernelGGL(envmap_eval_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, E, a.as<float>(), n, v.as<float>(), q.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return v.download(ctx, out_rgb, n * 12) || q.download(ctx, out_pdf, n * 4);
}
int mer_envmap_sample(mer_context *ctx, const mer_scene_desc *scene, const float *u2, int64_t n, float *out_dir, float *out_value_over_pdf, float *out_pdf) {
    MER_USE_DEVICE(ctx);
    Params P;
    const DEnvMap *E = envmap_of(ctx, scene, P, "mer_envmap_sample");
    if (!E) return 1;
    if (n <= 0) return 0;
    DeviceBuffer a, d, v, q;
    if (a.upload(ctx, u2, n * 8) || d.alloc(ctx, n * 12) || v.alloc(ctx, n * 12) || q.alloc(ctx, n * 4)) return 1;
    hipLaunchKernelGGL(envmap_sample_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, E, a.as<float>(), n, d.as<float>(), v.as<float>(), q.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return d.download(ctx, out_dir, n * 12) || v.download(ctx, out_value_over_pdf, n * 12) || q.download(ctx, out_pdf, n * 4);
}
int mer_rough_dielectric_eval(mer_context *ctx, const mer_scene_desc *scene, const float *eta, const float *wi, const float *wo, int64_t n,
                              float *out_val, float *out_pdf) {
    MER_USE_DEVICE(ctx);
    if (check_rough(ctx, scene)) return 1;
    DeviceBuffer a, b, c, e, f;
    if (a.upload(ctx, eta, n * 4) || b.upload(ctx, wi, n * 12) || c.upload(ctx, wo, n * 12) || e.alloc(ctx, n * 4) || f.alloc(ctx, n * 4)) return 1;
    hipLaunchKernelGGL(rough_eval_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, scene->rough_distribution, scene->rough_alpha,
                       scene->rough_sample_visible, a.as<float>(), b.as<float>(), c.as<float>(), n, e.as<float>(), f.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    if (e.download(ctx, out_val, n * 4)) return 1;
    return f.download(ctx, out_pdf, n * 4);
}
int mer_rough_dielectric_sample(mer_context *ctx, const mer_scene_desc *scene, const float *eta, const float *wi, const float *u3, int64_t n,
                                float *wo, float *weight, float *pdf) {
    MER_USE_DEVICE(ctx);
    if (check_rough(ctx, scene)) return 1;
    DeviceBuffer a, b, c, e, f, g;
    if (a.upload(ctx, eta, n * 4) || b.upload(ctx, wi, n * 12) || c.upload(ctx, u3, n * 12) || e.alloc(ctx, n * 12) || f.alloc(ctx, n * 4) || g.alloc(ctx, n * 4)) return 1;
    hipLaunchKernelGGL(rough_sample_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, scene->rough_distribution, scene->rough_alpha,
                       scene->rough_sample_visible, a.as<float>(), b.as<float>(), c.as<float>(), n, e.as<float>(), f.as<float>(), g.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    if (e.download(ctx, wo, n * 12) || f.download(ctx, weight, n * 4)) return 1;
    return g.download(ctx, pdf, n * 4);
}
int mer_camera_rays(mer_context *ctx, const mer_scene_desc *scene, const float *pos2, int64_t n, float *o, float *d) {
    MER_USE_DEVICE(ctx);
    Params P;
    mer_scene_desc sc = sensor_fields_only(*scene);
    if (make_params(ctx, &sc, P)) return 1;
    DeviceBuffer a, b, c;
    if (a.upload(ctx, pos2, n * 8) || b.alloc(ctx, n * 12) || c.alloc(ctx, n * 12)) return 1;
    hipLaunchKernelGGL(camera_rays_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P, a.as<float>(), n, b.as<float>(), c.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    if (b.download(ctx, o, n * 12)) return 1;
    return c.download(ctx, d, n * 12);
}
int mer_sensor_rays(mer_context *ctx, const mer_scene_desc *scene, const float *pos2, const float *aperture2, int64_t n, float *o, float *d,
                    float *mint, float *maxt) {
    MER_USE_DEVICE(ctx);
    Params P;
    mer_scene_desc sc = sensor_fields_only(*scene);
    if (make_params(ctx, &sc, P)) return 1;
    const bool lens = sc.sensor == MER_SENSOR_THINLENS || sc.sensor == MER_SENSOR_TELECENTRIC;
    if (lens && !aperture2) return fail(ctx, "mer_sensor_rays: a thinlens / telecentric sensor needs the aperture samples");
    DeviceBuffer a, u, b, c, e, f;
    if (a.upload(ctx, pos2, n * 8) || b.alloc(ctx, n * 12) || c.alloc(ctx, n * 12) || e.alloc(ctx, n * 4) || f.alloc(ctx, n * 4)) return 1;
    if (lens && u.upload(ctx, aperture2, n * 8)) return 1;
    hipLaunchKernelGGL(sensor_rays_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P, a.as<float>(), lens ? u.as<float>() : (const float *) nullptr, n,
                       b.as<float>(), c.as<float>(), e.as<float>(), f.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    if (b.download(ctx, o, n * 12) || c.download(ctx, d, n * 12) || e.download(ctx, mint, n * 4)) return 1;
    return f.download(ctx, maxt, n * 4);
}
int mer_correlation(mer_context *ctx, const mer_scene_desc *scene, const float *path_length, int64_t n, float *out) {
    MER_USE_DEVICE(ctx);
    Params P;
    mer_scene_desc sc = sensor_fields_only(*scene);
    if (make_params(ctx, &sc, P)) return 1;
    if (sc.modulation == MER_MODULATION_NONE) return fail(ctx, "Cannot call correlation function when the modulation type is not defined");   // pathlengthsampler.cpp:71-73
    DeviceBuffer a, b;
    if (a.upload(ctx, path_length, n * 4) || b.alloc(ctx, n * 4)) return 1;
    hipLaunchKernelGGL(correlation_kernel, dim3(nblocks(n)), dim3(256), 0, ctx->stream, P, a.as<float>(), n, b.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return b.download(ctx, out, n * 4);
}
int mer_rng_floats(mer_context *ctx, uint64_t seed, uint32_t pixel, uint32_t sample, int32_t n, float *out) {
    MER_USE_DEVICE(ctx);
    DeviceBuffer a;
    if (a.alloc(ctx, (size_t) n * 4)) return 1;
    hipLaunchKernelGGL(rng_kernel, dim3(1), dim3(64), 0, ctx->stream, seed, pixel, sample, n, a.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    return a.download(ctx, out, (size_t) n * 4);
}
int mer_synth_field_dev(mer_context *ctx, int32_t kind, int32_t N, float **data_dev) {
    MER_USE_DEVICE(ctx);
    if (kind < 0 || kind > 2 || N < 2) return fail(ctx, "mer_synth_field_dev: bad arguments");
    DeviceBuffer field;              // the caller's on success (mer_device_free)
    if (field.alloc(ctx, (size_t) N * N * N * 4)) return 1;
    hipLaunchKernelGGL(synth_field_kernel, dim3(8192), dim3(256), 0, ctx->stream, kind, N, field.as<float>());
    HIP_CHECK(ctx, hipGetLastError());
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    *data_dev = (float *) field.release();
    return 0;
}

}  // extern "C"
