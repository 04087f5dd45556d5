// mer_internal.hpp -- host-side state of libmer.so shared by its translation units (mer_api.hip: context, volumes, film, leaf entry
// points; mer_scene.hip: scene flattening, make_params; mer_render.hip: the wavefront host loop; mer_render_*.hip: the kernel
// instantiations, one group per file so that they compile in parallel).  Nothing here is part of the C-ABI (include/mer.h).
#pragma once
#include "mer_device.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <cmath>
#include <string>
#include <vector>
#include <map>
#include <limits>

struct mer_context;

namespace mer {

// The one owner of device memory: a pointer and its capacity in bytes, freed by the destructor (on whatever device is current: every
// entry point, mer_context_destroy included, selects the context's device first).  Move-only.  alloc / reserve / upload / download
// return the usual int with the context's error set (defined below HIP_CHECK); no other code allocates or frees.
struct DeviceBuffer {
    void *p = nullptr; size_t bytes = 0;
    DeviceBuffer() = default;
    DeviceBuffer(DeviceBuffer &&o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DeviceBuffer &operator=(DeviceBuffer &&o) noexcept { if (this != &o) { reset(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; } return *this; }
    ~DeviceBuffer() { reset(); }
    void reset() { if (p) (void) hipFree(p); p = nullptr; bytes = 0; }
    void *release() { void *q = p; p = nullptr; bytes = 0; return q; }          // to a caller of the C-ABI, who frees it with free_raw
    static int free_raw(mer_context *ctx, void *raw);
    int alloc(mer_context *ctx, size_t n);                   // a fresh buffer of n bytes (at least 4), whatever was held before
    int reserve(mer_context *ctx, size_t n) { return p && bytes >= n ? 0 : alloc(ctx, n); }      // grows, never shrinks; contents are not kept
    int upload(mer_context *ctx, const void *host, size_t n);      // alloc + copy on the context stream
    int download(mer_context *ctx, void *host, size_t n) const;    // copy on the context stream + synchronise
    template <typename T> T *as() const { return (T *) p; }
    explicit operator bool() const { return p != nullptr; }
};
struct PinnedBuffer {              // its pinned-host twin (Pipe::host_live): allocated once, never moved
    void *p = nullptr;
    PinnedBuffer() = default;
    PinnedBuffer(const PinnedBuffer &) = delete;
    ~PinnedBuffer() { if (p) (void) hipHostFree(p); }
    int alloc(mer_context *ctx, size_t n);
};

struct Volume {
    mer_grid_desc desc;
    DeviceBuffer dense;         // dense layout
    DeviceBuffer cell8;         // CELL8 / BRICK records (optional)
    DeviceBuffer coeff;         // B-spline coefficients (optional)
    int layout = MER_LAYOUT_DENSE;
    size_t bytes_dense = 0;
};

// emitter `envmap` (mer_envmap_upload): one device buffer -- texels [h][w] (4 x fp16), then the float tables cdf_cols [h][w + 1], cdf_rows [h + 1],
// row_weights [h] at the given byte offsets -- and the normalisation.  Its handle shares the volumes' numbering.
struct EnvMap {
    DeviceBuffer dev;
    int32_t w = 0, h = 0;
    float norm = 0;
    size_t off_cols = 0, off_rows = 0, off_weights = 0;
};

// what a light-path render records into (mer_fluence_create / _track_create / _time_create, mer_exitance_create, mer_sensitivity_create): one device
// buffer -- n_keys x 3 float64 sums, then n_totals totals -- and what the launch needs to fill it.  Handles share the volumes' numbering and one map;
// the family decides which entry points know a handle (the other two families refuse it as unknown), the kind which kernel a fluence handle renders with.
//   fluence      sums [frames][nz][ny][nx][3] over `box`, 8 totals; timed: frames > 0 bins of det.t_bin from det.t_min on, 12 totals; track: K_fluence_track
//   exitance     sums [frames][faces][res_v][res_u][3], 16 totals: det holds the boundary, raster, window and cone
//   REC_FD       a fluence grid or an exitance map with 2 x n_freq planes in place of the frames (real, imaginary per frequency), no window, the totals
//                of its steady sibling; the wavenumbers, float64[MER_MAX_FREQUENCIES], lie behind the totals, where the kernels read them (a
//                clear leaves them alone)
//   sensitivity  sums [1 + scatter][gates][ndv][ndu][nz][ny][nx][3] over `box`, 16 totals, then n_meas = gates x ndv x ndu measurements of 8 float64:
//                det is the raster, window, cone and first gate; one detector is bin_u x bin_v cells of the window (mer_sensitivity_create: all of it)
enum { REC_FLUENCE = 0, REC_EXITANCE = 1, REC_SENSITIVITY = 2 };      // Recorder::family
enum { REC_COLLISION = 0, REC_TRACK = 1, REC_TIMED = 2, REC_FD = 3 };  // Recorder::kind (fluence: all four; exitance: the first -- steady or gated -- and REC_FD; sensitivity: the first)
struct Recorder {
    int32_t family = REC_FLUENCE, kind = REC_COLLISION;
    mer_fluence_desc box{};
    mer_detector_desc det{};
    int32_t frames = 0;                          // 0: a steady-state fluence grid, a sensitivity grid
    DeviceBuffer dev;
    uint64_t n_keys = 0;
    int32_t n_totals = 0;                        // as allocated: 8 or 12 (timed) for fluence, 16 for the others
    int32_t bin_u = 0, bin_v = 0, gates = 1, scatter = 0;      // sensitivity
    uint64_t n_meas = 0;                         // sensitivity: the measurements, 8 float64 each behind the totals
    int32_t n_freq = 0; double wavenumber[MER_MAX_FREQUENCIES] = {};     // REC_FD: the wavenumbers (the host's copy)
    bool timed() const { return kind == REC_TIMED; }
    bool fd() const { return kind == REC_FD; }
    bool track() const { return kind == REC_TRACK; }
    uint64_t n_cells() const { return (uint64_t) box.res[0] * (uint64_t) box.res[1] * (uint64_t) box.res[2]; }
    int32_t faces() const { return det.boundary == MER_BOUNDARY_SPHERE ? 1 : 6; }
    double *sums() const { return dev.as<double>(); }
    double *totals() const { return sums() + n_keys * 3; }
    double *meas() const { return totals() + n_totals; }
    double *wavenumbers() const { return totals() + n_totals; }        // REC_FD (which has no measurements)
    size_t cleared_bytes() const { return (n_keys * 3 + (uint64_t) n_totals + n_meas * 8) * sizeof(double); }      // what a clear zeroes
    size_t bytes() const { return cleared_bytes() + (fd() ? sizeof(wavenumber) : 0); }
};

#define MER_MAX_PIPES 4
struct Pipe {
    hipStream_t stream = nullptr, own_stream = nullptr;      // pipeline 0 runs on the context stream
    // the pool (prepare_pool, mer_render.hip): nslots counts RECORDS (path slots + side-walk slots); the lists hold record ids and are sized by it
    DeviceBuffer slots; uint32_t nslots = 0; DeviceBuffer live; PinnedBuffer host_live;
    // the seven work lists in one order -- eq, mq[0], mq[1], sq[0], sq[1], cq[0], cq[1] -- as the kernels see them (raw pointers, copied into Params)
    // and the owners of their arrays beside them
    enum { NQ = 7, EQ = 0, MQ = 1, SQ = 3, CQ = 5 };
    SegQueue q[NQ]{};
    DeviceBuffer q_items[NQ], q_counts[NQ], q_keys[NQ];           // keys: the march lists only, with the first render that sorts them
    DeviceBuffer cstate;                                          // parked solver states of K_connect, one per record (allocated on first use)
    DeviceBuffer hitq, hitq_ctr; unsigned long long hitq_cap = 0;
    hipEvent_t readback[2] = {nullptr, nullptr}, finished = nullptr;     // two batches in flight per pipeline
    std::vector<hipEvent_t> pass_events;          // 3 per pass: before K_event, between, after K_march
    DeviceBuffer side_state;                                      // busy bytes of the side-walk slots, 8 per path slot (allocated with the first render that spawns)
    DeviceBuffer msort;                                           // spatial sort of the march list: sorted ids (one per record), histogram, cursors, count
};

// Tuning / A-B switches of a context (mer_context_set_option).  Defaults are the measured optima of DESIGN.md section 4.
struct Options {
    int64_t pipes = 4;            // concurrent pipelines per render (1..MER_MAX_PIPES)
    int64_t nslots = 0;           // path-state slots over all pipelines; 0 = 4 x the resident lanes of the chip
    int64_t ksteps = 128;         // eikonal steps / tentative collisions per lane per K_march launch
    int64_t mq_sort = -1;         // march lists sorted by steps-to-boundary class: -1 = by field size, 0 / 1 = off / on
    int64_t connect_launches = 2;    // K_connect launches per pass (one solver unit per pending connection per launch; 1-3 measured equal, 6+ slower)
    int64_t adaptive_k = 0;       // pass length in the tail of a render: 0 fixed (default), 1 longer (rounds 1-2: measured a loss), 2 shorter
    int64_t pass_events = 1;      // per-pass HIP events (mer_last_render_stats)
    int64_t buffer_loads = 1;     // 0: global loads even for fields below 4 GiB (the kernels a >= 4 GiB field selects)
    int64_t gen_all = 0;          // K_gen hands every camera sample to K_event (A/B)
    int64_t prefilter = 0;        // K_prefilter form: 0 register windows, 1 one thread per line, 2 two kernels per axis, 3 strided x pass, 4 LDS x pass
    int64_t verbose = 0;
    int64_t debug_pixel = -1;
    int64_t march_lds_kb = 0;     // KiB of (unused) dynamic LDS per K_march block: caps its occupancy (160 KiB per CU; 33 -> 4 blocks, 41 -> 3) for A/B runs
    int64_t tile_deal = 1;        // tile shards dealt on diagonals (1, default) or in plain row-major round robin (0): decode_work
    int64_t inline_walks = 1;     // straight rays in a gridded sigma_t: K_event runs the walks itself (persistent lanes) instead of handing them to K_march
    int64_t spawn_walks = 1;      // curved rays, steady-state film: luminaire-sample / look-up walks run in side-walk slots while the path goes on (mer_wavefront.hpp)
    int64_t small_render_slots = 1;   // a render with few paths per slot uses fewer slots / pipelines, so that the wavefront stays full while it drains
    int64_t check_every = 4;      // passes per batch: the host reads the finished-slot count back once per batch, two batches in flight per pipeline (8 until round 3: 4 is +4 % on configs[1], +1 % on small renders, neutral on long ones)
    int64_t grid_fit = 1;         // launch grids sized by what the lists can still hold (live path slots x records per path + side walks in flight at the last read-back) instead of by every record
    int64_t march_sort = 0;       // curved rays, record layouts: march list also sorted by position (bits per axis of the cell grid, 1..3; 0 = off) and swept in XCD-contiguous chunks
    int64_t march_sort_major = 0; // bin order of that sort: 0 = cell-major (all exit-time classes of a cell together), 1 = class-major
    int64_t lds_bricks = 0;       // K_march keeps every lane's current BRICK27 record in LDS (BRICK27 below 4 GiB only; measured slower)
};

}  // namespace mer

struct mer_context {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string error;
    std::map<int, mer::Volume> volumes;
    std::map<int, mer::EnvMap> envmaps;          // mer_envmap_upload (handles from next_handle, as the volumes')
    std::map<int, mer::Recorder> recorders;      // fluence grids, exitance maps, sensitivity grids (handles from next_handle)
    mer::DeviceBuffer detect_list; uint32_t detect_cap = 0;   // the detected-path list of mer_render_sensitivity (allocated on first use): 64 words whose first is the count, then 5 arrays of detect_cap words
    int next_handle = 1;
    mer::DeviceBuffer counters;                  // MER_C_COUNT x replicas + work counter
    mer::DeviceBuffer ftable; int ftable_kind = -1; float ftable_param = 0;   // reconstruction-filter table on the device (33 floats) and what it holds
    // the emitter table on the device (points, rectangles, spot cones, the envmap record: mer_device.hpp) and the value it holds, once uploaded
    mer::DeviceBuffer etab; mer::EmitterTable etab_host; bool etab_valid = false;
    mer::DeviceBuffer chk_buf;                   // MER_BOUNDS_CHECK build: violation record (count, kind, index, limit) ...
    unsigned long long *chk = nullptr;           // ... as every kernel argument carries it (null in the plain build)
    hipEvent_t ev0 = nullptr, ev1 = nullptr;
    bool timed = false;
    hipDeviceProp_t prop;
    mer::Options opt;
    // wavefront pipelines: path-state slots, work lists, hit ring, work counter and stream of each (launch_render)
    mer::Pipe pipes[MER_MAX_PIPES];
    int last_passes = 0, last_pipes = 1;
    float last_march_ms = 0, last_event_ms = 0;
};

#define HIP_CHECK(ctx, call)                                                                              \
    do {                                                                                                  \
        hipError_t e_ = (call);                                                                           \
        if (e_ != hipSuccess) {                                                                           \
            (ctx)->error = std::string(#call) + " failed: " + hipGetErrorString(e_);                      \
            return 1;                                                                                     \
        }                                                                                                 \
    } while (0)

namespace mer {

inline int DeviceBuffer::free_raw(mer_context *ctx, void *raw) { HIP_CHECK(ctx, hipFree(raw)); return 0; }
inline int DeviceBuffer::alloc(mer_context *ctx, size_t n) {
    reset();
    HIP_CHECK(ctx, hipMalloc(&p, n ? n : 4));
    bytes = n;
    return 0;
}
inline int DeviceBuffer::upload(mer_context *ctx, const void *host, size_t n) {
    if (alloc(ctx, n)) return 1;
    if (n) HIP_CHECK(ctx, hipMemcpyAsync(p, host, n, hipMemcpyHostToDevice, ctx->stream));
    return 0;
}
inline int DeviceBuffer::download(mer_context *ctx, void *host, size_t n) const {
    if (n) HIP_CHECK(ctx, hipMemcpyAsync(host, p, n, hipMemcpyDeviceToHost, ctx->stream));
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));
    return 0;
}
inline int PinnedBuffer::alloc(mer_context *ctx, size_t n) { HIP_CHECK(ctx, hipHostMalloc(&p, n)); return 0; }

static inline int fail(mer_context *ctx, const std::string &msg) { ctx->error = msg; return 1; }
static inline unsigned nblocks(int64_t n, int bs = 256) { return (unsigned) std::max<int64_t>(1, (n + bs - 1) / bs); }

// the scene of a leaf entry point that reads the sensor fields only: no volume is looked up
static inline mer_scene_desc sensor_fields_only(mer_scene_desc sc) { sc.sigma_mode = MER_SIGMA_HOMOGENEOUS; sc.rif_mode = MER_RIF_CONST; sc.albedo_mode = MER_ALBEDO_CONST; return sc; }

// mer_scene.hip: scene flattening (host only)
// linear part of a row-major 3x4 float matrix in double; determinant and inverse (returns the determinant) of a 3x3 matrix by cofactors
static inline void linear3(const float m[12], double M[3][3]) { for (int i = 0; i < 3; i++) for (int j = 0; j < 3; j++) M[i][j] = m[4 * i + j]; }
double det3(const double M[3][3]);
double inverse3(const double M[3][3], double inv[3][3]);
// records = false: the dense data even where the volume has a record layout (spectrum look-ups, the albedo)
void fill_dgrid(const mer_context *ctx, const Volume &v, DGrid &g, bool records = true);
// point_outside (optional): a point emitter of the scene lies outside the cube / sphere medium shape (launch_render picks the connect kernel by it)
int make_params(mer_context *ctx, const mer_scene_desc *sc, Params &P, bool allow_sdf = false, bool *point_outside = nullptr);
int film_frames(mer_context *ctx, const mer_scene_desc *sc, int &frames);
int check_rough(mer_context *ctx, const mer_scene_desc *sc);
// internal fetch kind (RIFK_*) of the scene's trilinear RIF volume, or the rif_mode itself for the other modes
int rif_fetch_kind(mer_context *ctx, const mer_scene_desc *sc);

// mer_render.hip: one render = a few independent pipelines of K_gen / K_event / [K_connect] / K_march passes
struct Run {
    Params P; uint32_t nslots = 0, pass = 0; unsigned blocks = 0, gen_blocks = 0;
    int cur = 0; bool work_left = true, done = false;
    uint32_t alive_bound = 0, child_bound = 0;      // from the last read-back: path slots not yet finished (never grows), side walks then in flight
};
// the kernels of one (CURVED, RIF, STEPPER, SIGMA, BND) combination, as launchable function pointers
typedef void (*GenKernel)(const Params);
typedef void (*PassKernel)(const Params, uint32_t);
struct KernelSet { GenKernel gen; PassKernel event, march, connect, connect_cross, march_lds, event_inline, event_rough, event_inline_rough; };   // event_rough / event_inline_rough: the K_event instances of a rough dielectric boundary   // event_inline: K_event that runs straight walks itself (or null)   // connect_cross: the point emitter lies outside the medium shape;
                                                                                                    // march_lds: K_march with LDS-staged BRICK27 records (or null)
// each mer_render_<group>.hip answers for the combinations it instantiates (returns false if the combination is not in its group)
bool kernels_straight(int sigma, int bnd, bool extra, KernelSet &k);
bool kernels_acoustic(int stepper, int sigma, bool extra, KernelSet &k);
bool kernels_dense(int rifk, int stepper, int sigma, bool extra, KernelSet &k);
bool kernels_cell8(int rifk, int stepper, int sigma, bool extra, KernelSet &k);
bool kernels_brick(int rifk, int stepper, int sigma, bool extra, KernelSet &k);
bool kernels_bspline(int stepper, int sigma, bool extra, KernelSet &k);
bool kernels_sdf_curved(int rifk, int stepper, int sigma, KernelSet &k);
bool kernels_sdf_curved_records(int rifk, int stepper, int sigma, KernelSet &k);      // BRICK27 (both load kinds), CELL8 with global loads
int tile_skew_for(int tiles_x, int tile_count, int tile_deal);
// the shard's check ("invalid shard") and the work fields of P: sample range, tile deal, total_work
int set_work(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, Params &P);
int launch_render(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, float *film_dev, float *path_out_dev,
                  uint64_t n_film, uint64_t n_path_out);

// mer_render_ptracer.hip: integrator = MER_INTEGRATOR_PTRACER -- one lane per light path, launched a fixed number of paths at a time
int launch_ptracer(mer_context *ctx, const mer_scene_desc *scene, const mer_shard *shard, uint64_t seed, float *film_dev, uint64_t n_film);

// mer_render_fluence.hip, mer_render_exitance.hip, mer_render_sensitivity.hip: what the same light paths record into a Recorder (above), each
// family's kernels, launch and entry points; what they share is mer_lightpath_host.hpp

// mer_sdf_build.hip: signed-distance grid of a triangle mesh.  tri12_host: 12 floats per triangle (3 vertices, xyz + one unused float each), already
// validated; on success sdf / winding hold one float per node (x fastest).
struct SdfGridArgs { int32_t res[3]; float lo[3], step[3]; uint64_t n_nodes; unsigned long long *chk; };
#define MER_SDF_DEFAULT_CHUNK 4096                         // triangles per launch when the caller passes 0
#define MER_SDF_NODES_PER_LAUNCH ((uint64_t) 1 << 24)      // nodes per launch (256^3): with the default chunk 6.9e10 pairs per launch
int sdf_build(mer_context *ctx, const mer_grid_desc *d, const float *tri12_host, int64_t n_tri, int32_t max_tri_per_launch, DeviceBuffer &sdf, DeviceBuffer &winding);

}  // namespace mer
