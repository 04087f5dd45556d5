// mer_scene.hip -- scene flattening, host only: a mer_scene_desc becomes the kernel argument Params and the context's device tables
// (reconstruction filter, emitters).  make_params is a sequence of steps, one per group of reference plugins; every step validates
// the way the plugins' constructors / configure() do and fails with their message.  No kernel lives here: the unit sees the device
// structs (mer_device.hpp through mer_internal.hpp) and nothing of mer_kernels.hpp.
#include "mer_internal.hpp"
#include <algorithm>
#include <functional>

namespace mer {

// determinant of a 3x3 matrix by the first row's cofactors, and inverse = adjugate / det (returns det; inv is meaningless when it is 0).
// Every host-derived inverse (volumes' toWorld, rectangles, spot cones, the envmap's rotation) uses these expressions, in double.
double det3(const double M[3][3]) {
    const double a = M[0][0], b = M[0][1], c = M[0][2], d = M[1][0], e = M[1][1], f = M[1][2], g = M[2][0], h = M[2][1], k = M[2][2];
    return a * (e * k - f * h) - b * (d * k - f * g) + c * (d * h - e * g);
}
double inverse3(const double M[3][3], double inv[3][3]) {
    const double a = M[0][0], b = M[0][1], c = M[0][2], d = M[1][0], e = M[1][1], f = M[1][2], g = M[2][0], h = M[2][1], k = M[2][2];
    const double det = det3(M);
    inv[0][0] = (e * k - f * h) / det; inv[0][1] = (c * h - b * k) / det; inv[0][2] = (b * f - c * e) / det;
    inv[1][0] = (f * g - d * k) / det; inv[1][1] = (a * k - c * g) / det; inv[1][2] = (c * d - a * f) / det;
    inv[2][0] = (d * h - e * g) / det; inv[2][1] = (b * g - a * h) / det; inv[2][2] = (a * e - b * d) / det;
    return det;
}

// what the kernels fetch a volume's values from: the layout they see, the brick geometry, the bytes of that buffer (dense data, CELL8
// cells or BRICK records) and the extent buffer loads use (0 = global loads: 4 GiB or more, or option buffer_loads = 0)
struct RecordInfo { int layout, bshift, recw, nbx, nby; uint64_t bytes; uint32_t buf_bytes; };
static RecordInfo record_info(const mer_context *ctx, const Volume &v, bool records = true) {
    RecordInfo r;
    records = records && v.cell8;
    r.layout = records ? v.layout : MER_LAYOUT_DENSE;
    const bool brick = records && (v.layout == MER_LAYOUT_BRICK27 || v.layout == MER_LAYOUT_BRICK125);
    r.bshift = v.layout == MER_LAYOUT_BRICK125 ? 2 : 1; r.recw = v.layout == MER_LAYOUT_BRICK125 ? 128 : 32;
    const int bc = 1 << r.bshift;                                       // ceil((res-1)/bc) bricks per axis
    r.nbx = (v.desc.res[0] - 2) / bc + 1; r.nby = (v.desc.res[1] - 2) / bc + 1;
    r.bytes = !records ? (uint64_t) v.bytes_dense
            : brick ? (uint64_t) r.nbx * r.nby * ((v.desc.res[2] - 2) / bc + 1) * (uint64_t) r.recw * 4ull
            : (uint64_t) (v.desc.res[0] - 1) * (v.desc.res[1] - 1) * (v.desc.res[2] - 1) * 32ull;
    r.buf_bytes = r.bytes < 0xFFFFFFFFull && ctx->opt.buffer_loads ? (uint32_t) r.bytes : 0u;
    return r;
}

// worldToGrid = scale((res-1)/extents) * translate(-min) * toWorld^-1 with toWorld = identity
// (GridDataSource::configure, src/volume/gridvolume.cpp:188-195).  Float arithmetic as in the reference.
void fill_dgrid(const mer_context *ctx, const Volume &v, DGrid &g, bool records) {
    std::memset(&g, 0, sizeof(g));
    records = records && v.cell8;
    g.data = v.dense.p; g.cell8 = records ? v.cell8.as<float>() : nullptr; g.coeff = v.coeff.as<float>();
    g.channels = v.desc.channels; g.dtype = v.desc.dtype;
    const RecordInfo r = record_info(ctx, v, records);
    g.layout = r.layout; g.bshift = r.bshift; g.bw = (1 << g.bshift) + 1; g.recw = r.recw; g.nbx = r.nbx; g.nby = r.nby;
    g.buf_bytes = r.buf_bytes;
    g.n_record = records ? r.bytes / 4 : 0;
    g.n_dense = (uint64_t) v.desc.res[0] * v.desc.res[1] * v.desc.res[2] * (uint64_t) v.desc.channels;
    g.chk = ctx->chk;
    // worldToVolume: the desc's matrix, all zeros = identity
    float W[12]; bool zero = true;
    for (int i = 0; i < 12; i++) { W[i] = v.desc.world_to_volume[i]; zero = zero && W[i] == 0.0f; }
    if (zero) for (int i = 0; i < 12; i++) W[i] = (i % 5 == 0) ? 1.0f : 0.0f;
    g.affine = 0;
    for (int i = 0; i < 12; i++) { g.w2v[i] = W[i]; if (W[i] != ((i % 5 == 0) ? 1.0f : 0.0f)) g.affine = 1; }
    for (int i = 0; i < 3; i++) {
        g.res[i] = v.desc.res[i];
        g.bmin[i] = v.desc.aabb_min[i]; g.bmax[i] = v.desc.aabb_max[i];
        const float extent = g.bmax[i] - g.bmin[i];
        const float s = (float) (g.res[i] - 1) / extent;
        g.s[i] = s;
        g.t[i] = s * (-g.bmin[i]);
        // (scale * translate) * worldToVolume as Mitsuba's 4x4 product forms it (src/libcore/transform.cpp operator*): row i of the
        // left factor is (s_i e_i, s_i * (-min_i)); the zero terms of the sums add exactly nothing
        for (int j = 0; j < 3; j++) g.m[i * 4 + j] = s * W[i * 4 + j];
        g.m[i * 4 + 3] = s * W[i * 4 + 3] + g.t[i];
        // SplineDataSource interpolatable limits (src/volume/splinevolume.cpp:280-281): stride = 1/xres
        const float stride = (float) (1.0 / s);
        g.lim_min[i] = g.bmin[i] + (2.0f * stride + MER_EPSILON);
        g.lim_max[i] = g.bmax[i] + (-2.0f * stride - MER_EPSILON);
    }
    {   // m_aabb: bounding box of the data box's corners under volumeToWorld (gridvolume.cpp:199-203); volumeToWorld = W^-1 by cofactors
        // in double (the oracle forms it with the same expressions)
        double A[3][3], inv[3][3];
        linear3(W, A);
        inverse3(A, inv);
        for (int i = 0; i < 3; i++) { g.wmin[i] = std::numeric_limits<float>::infinity(); g.wmax[i] = -std::numeric_limits<float>::infinity(); }
        for (int corner = 0; corner < 8; corner++) {
            const double q[3] = {((corner & 1) ? g.bmax[0] : g.bmin[0]) - (double) W[3], ((corner & 2) ? g.bmax[1] : g.bmin[1]) - (double) W[7],
                                 ((corner & 4) ? g.bmax[2] : g.bmin[2]) - (double) W[11]};
            for (int i = 0; i < 3; i++) {
                const float w = (float) (inv[i][0] * q[0] + inv[i][1] * q[1] + inv[i][2] * q[2]);
                g.wmin[i] = std::min(g.wmin[i], w); g.wmax[i] = std::max(g.wmax[i], w);
            }
        }
    }
}

int rif_fetch_kind(mer_context *ctx, const mer_scene_desc *sc) {
    if (sc->rif_mode != MER_RIF_TRILINEAR) return sc->rif_mode;
    const RecordInfo r = record_info(ctx, ctx->volumes.find(sc->rif)->second);
    if (r.layout == MER_LAYOUT_BRICK27 || r.layout == MER_LAYOUT_BRICK125) return r.buf_bytes ? RIFK_BRICK27_BUF : RIFK_BRICK27;
    if (r.layout == MER_LAYOUT_CELL8) return r.buf_bytes ? RIFK_CELL8_BUF : RIFK_CELL8;
    return r.buf_bytes ? RIFK_DENSE_BUF : MER_RIF_TRILINEAR;
}

static void filter_table(int kind, float param, float *values, float &radius, float &scale) {
    // ReconstructionFilter::configure (src/libcore/rfilter.cpp:40-55), MTS_FILTER_RESOLUTION = 31
    const int RES = 31;
    radius = kind == MER_FILTER_BOX ? param + 1e-5f : 4 * param;      // box.cpp:39, gaussian.cpp:42
    float sum = 0.0f;
    for (int i = 0; i < RES; ++i) {
        const float x = (radius * i) / RES;
        float v;
        if (kind == MER_FILTER_BOX) v = std::fabs(x) <= radius ? 1.0f : 0.0f;
        else {
            const float alpha = -1.0f / (2.0f * param * param);
            v = std::max(0.0f, std::exp(alpha * x * x) - std::exp(alpha * radius * radius));
        }
        values[i] = v; sum += v;
    }
    values[RES] = 0.0f; values[RES + 1] = 0.0f;
    scale = RES / radius;
    sum *= 2 * radius / RES;
    const float normalization = 1.0f / sum;
    for (int i = 0; i < RES; ++i) values[i] *= normalization;
}

int film_frames(mer_context *ctx, const mer_scene_desc *sc, int &frames) {
    frames = 1;
    if (sc->modulation < MER_MODULATION_NONE || sc->modulation > MER_MODULATION_DEPTHSELECTIVE)            // pathlengthsampler.cpp:33-35
        return fail(ctx, "The \"modulation\" parameter must be equal toeither \"none\", \"square\", or \"hamiltonian\", or \"mseq\", or \"depthselective\"!");
    if (sc->modulation != MER_MODULATION_NONE && sc->decomposition != MER_DECOMPOSITION_TRANSIENT)
        return fail(ctx, "film: a path-length modulation needs decomposition = transient");
    if (sc->modulation != MER_MODULATION_NONE && (!(sc->mod_lambda > 0) || sc->mod_P < 1 || sc->mod_neighbors < 0))
        return fail(ctx, "film: modulation needs lambda > 0, P >= 1, neighbors >= 0");
    if (sc->decomposition == MER_DECOMPOSITION_NONE) return 0;
    if (sc->decomposition == MER_DECOMPOSITION_TRANSIENT && sc->modulation != MER_MODULATION_NONE) return 0;  // film.cpp:76-78: one frame
    if (sc->decomposition != MER_DECOMPOSITION_TRANSIENT && sc->decomposition != MER_DECOMPOSITION_BOUNCE)
        return fail(ctx, "The \"decomposition\" parameter must be equal toeither \"none\", \"transient\", or \"bounce\"!");   // film.cpp:66-68
    const float f = std::ceil((sc->max_bound - sc->min_bound) / sc->bin_width);                                               // film.cpp:74
    if (!(f >= 1.0f) || f > 4096.0f) return fail(ctx, "film: a decomposition needs 1 <= ceil((maxBound-minBound)/binWidth) <= 4096 frames");
    frames = (int) f;
    return 0;
}
// the microfacet parameters of MER_BSDF_HROUGHDIELECTRIC (microfacet.h:100-142: one isotropic alpha, clamped to >= 1e-4 on the device)
int check_rough(mer_context *ctx, const mer_scene_desc *sc) {
    if (sc->rough_distribution < MER_MICROFACET_BECKMANN || sc->rough_distribution > MER_MICROFACET_PHONG)
        return fail(ctx, "hroughdielectric: distribution must be beckmann, ggx or phong");
    if (!(sc->rough_alpha >= 0) || !std::isfinite(sc->rough_alpha)) return fail(ctx, "hroughdielectric: alpha must be finite and >= 0");
    if (sc->rough_sample_visible != 0 && sc->rough_sample_visible != 1) return fail(ctx, "hroughdielectric: sampleVisible must be 0 or 1");
    return 0;
}

// ---- emitters ---------------------------------------------------------------------------------------------------------------------

// inside test of the cube / sphere medium shape (heterogeneousrefractive.cpp:707-726), as the host applies it to an emitter position
static bool point_in_box(const mer_scene_desc &sc, const float q[3]) { bool in = true; for (int i = 0; i < 3; i++) in = in && q[i] >= sc.bmin[i] && q[i] <= sc.bmax[i]; return in; }
static bool point_in_sphere(const mer_scene_desc &sc, const float q[3]) { float d2 = 0; for (int i = 0; i < 3; i++) d2 += (q[i] - sc.sph_center[i]) * (q[i] - sc.sph_center[i]); return d2 < sc.sph_radius * sc.sph_radius; }
static bool point_in_shape(const mer_scene_desc &sc, const float q[3]) {
    if (sc.boundary == MER_BOUNDARY_AABB) return point_in_box(sc, q);
    if (sc.boundary == MER_BOUNDARY_SPHERE) return point_in_sphere(sc, q);
    return false;
}
// the signed-distance grid's trilinear value at q is negative (sdf_value); off the grid counts as outside
static int point_in_sdf(mer_context *ctx, const DGrid &g, const float q[3], bool &inside) {
    inside = false;
    float c[3];
    for (int i = 0; i < 3; i++) c[i] = g.m[4 * i] * q[0] + g.m[4 * i + 1] * q[1] + g.m[4 * i + 2] * q[2] + g.m[4 * i + 3];
    const int x1 = (int) std::floor(c[0]), y1 = (int) std::floor(c[1]), z1 = (int) std::floor(c[2]);
    if (!(x1 >= 0 && y1 >= 0 && z1 >= 0 && x1 < g.res[0] - 1 && y1 < g.res[1] - 1 && z1 < g.res[2] - 1)) return 0;
    float v = 0;
    for (int k = 0; k < 8; k++) {
        const int dx = k & 1, dy = (k >> 1) & 1, dz = k >> 2;
        float corner;
        HIP_CHECK(ctx, hipMemcpy(&corner, (const float *) g.data + ((size_t) (z1 + dz) * g.res[1] + (y1 + dy)) * g.res[0] + (x1 + dx), 4, hipMemcpyDeviceToHost));
        const float fx = c[0] - x1, fy = c[1] - y1, fz = c[2] - z1;
        v += (dx ? fx : 1 - fx) * (dy ? fy : 1 - fy) * (dz ? fz : 1 - fz) * corner;
    }
    inside = v < 0;
    return 0;
}
// A rough boundary samples the emitter from the surface vertex, so a point-table record must lie outside the medium shape.  Called where
// a record is added (cube / sphere; sdf = NULL) and, for a signed-distance shape, where its grid becomes known (boundary_shape).
static int refuse_inside_rough(mer_context *ctx, const mer_scene_desc &sc, const DGrid *sdf, const float pos[3], bool spot, const std::string &at) {
    if (sc.boundary_bsdf != MER_BSDF_HROUGHDIELECTRIC) return 0;
    bool inside = point_in_shape(sc, pos);
    if (sdf && point_in_sdf(ctx, *sdf, pos, inside)) return 1;
    if (!inside) return 0;
    return fail(ctx, at + (spot ? "hroughdielectric: the spot emitter must lie outside the medium shape (a curved connection that starts on the boundary is not built)"
                                : "hroughdielectric: the point emitter must lie outside the medium shape (a curved connection that starts on the boundary is not built)"));
}

// The scene's emitter records while they are built: the table that goes to device memory, how many slots of it are filled, and the
// sampling weights of the point and rectangle slots
struct Emitters {
    EmitterTable tab;
    int n_point = 0, n_rect = 0;
    bool any_spot = false, has_env = false;
    double wp[MER_MAX_EMITTERS], wr[MER_MAX_EMITTERS];
};

// objectToWorld (row-major 3x4, also returned in M), its inverse and the frame normal toWorld(Normal(0,0,1)) of a planar shape; returns the
// determinant of the linear part (0: singular, nothing else is valid)
static double frame_derive(const float to_world[12], DRect &R, double M[3][4]) {
    double A[3][3], inv[3][3];
    for (int i = 0; i < 12; i++) { R.o2w[i] = to_world[i]; M[i / 4][i % 4] = to_world[i]; }
    linear3(to_world, A);
    const double det = inverse3(A, inv);
    if (!(std::fabs(det) > 0)) return 0;
    for (int i = 0; i < 3; i++) {
        for (int j = 0; j < 3; j++) R.w2o[4 * i + j] = (float) inv[i][j];
        R.w2o[4 * i + 3] = (float) -(inv[i][0] * M[0][3] + inv[i][1] * M[1][3] + inv[i][2] * M[2][3]);
    }
    const double nn[3] = {inv[2][0], inv[2][1], inv[2][2]}, ln = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);   // o2w(Normal(0,0,1)): inverse transpose
    for (int i = 0; i < 3; i++) R.n[i] = (float) (nn[i] / ln);
    return det;
}
static double col_length(const double M[3][4], int c) { return std::sqrt(M[0][c] * M[0][c] + M[1][c] * M[1][c] + M[2][c] * M[2][c]); }
static double col_dot(const double M[3][4], int a, int b) { return M[0][a] * M[0][b] + M[1][a] * M[1][b] + M[2][a] * M[2][b]; }
// Rectangle::configure (src/shapes/rectangle.cpp:99-110): the frame and 1 / area of the image of [-1,1]^2 x {0}.  Returns an error message
// or nullptr.
static const char *rect_derive(const float to_world[12], DRect &R, double M[3][4]) {
    if (frame_derive(to_world, R, M) == 0) return "area emitter: 'toWorld' is singular";
    const double du[3] = {2 * M[0][0], 2 * M[1][0], 2 * M[2][0]}, dv[3] = {2 * M[0][1], 2 * M[1][1], 2 * M[2][1]};
    const double lu = std::sqrt(du[0] * du[0] + du[1] * du[1] + du[2] * du[2]), lv = std::sqrt(dv[0] * dv[0] + dv[1] * dv[1] + dv[2] * dv[2]);
    if (std::fabs((du[0] * dv[0] + du[1] * dv[1] + du[2] * dv[2]) / (lu * lv)) > MER_EPSILON) return "Error: 'toWorld' transformation contains shear!";    // :108-109
    R.inv_area = (float) (1.0 / (lu * lv));
    R.shape = AREA_RECT;
    return nullptr;
}
// Disk::configure (src/shapes/disk.cpp:101-115): the frame and 1 / area = 1 / (pi |dpdu|^2) of the image of the unit disk in z = 0
static const char *disk_derive(const float to_world[12], DRect &R, double M[3][4]) {
    if (frame_derive(to_world, R, M) == 0) return "area emitter: 'toWorld' is singular";
    const double lu = col_length(M, 0), lv = col_length(M, 1);
    if (std::fabs(col_dot(M, 0, 1) / (lu * lv)) > 1e-3) return "Error: 'toWorld' transformation contains shear!";                     // :108-109
    if (std::fabs(lu / lv - 1) > 1e-3) return "Error: 'toWorld' transformation contains a non-uniform scale!";                        // :111-112
    R.inv_area = (float) (1.0 / (M_PI * lu * lu));
    R.shape = AREA_DISK;
    return nullptr;
}
// Sphere's constructor (src/shapes/sphere.cpp:108-132): centre = the translation column, radius = |toWorld e_x|; the rotation is not kept.  A
// linear part of negative determinant means inward normals (flipNormals).  The reference reads the scale off e_x alone; here a linear part
// that is no uniform scale of a rotation (column lengths or angles off by more than 1e-3) is refused.
static const char *sphere_derive(const float to_world[12], DRect &R, double M[3][4]) {
    const double det = frame_derive(to_world, R, M);
    if (det == 0) return "area emitter: 'toWorld' is singular";
    const double l[3] = {col_length(M, 0), col_length(M, 1), col_length(M, 2)};
    for (int a = 0; a < 3; a++) {
        const int b = (a + 1) % 3;
        if (std::fabs(l[a] / l[b] - 1) > 1e-3 || std::fabs(col_dot(M, a, b) / (l[a] * l[b])) > 1e-3) return "sphere: 'toWorld' transformation contains a non-uniform scale!";
    }
    R.radius = (float) l[0];
    R.flip = det < 0 ? -1.0f : 1.0f;
    R.inv_area = (float) (1.0 / (4 * M_PI * l[0] * l[0]));
    R.shape = AREA_SPHERE;
    return nullptr;
}

// Exact test that the rectangle O + a U + b V (a, b in [-1, 1]; U = column 0, V = column 1, O = column 3 of M; U orthogonal to V) meets
// the closed medium shape.  Sphere: its point closest to the centre lies inside.  Cube: no separating axis among the box axes, the
// rectangle's edges and normal, and the nine edge-by-edge cross products.
static bool rect_meets_shape(const mer_scene_desc &sc, const double M[3][4]) {
    const double U[3] = {M[0][0], M[1][0], M[2][0]}, V[3] = {M[0][1], M[1][1], M[2][1]}, O[3] = {M[0][3], M[1][3], M[2][3]};
    auto dot3 = [](const double *a, const double *b) { return a[0] * b[0] + a[1] * b[1] + a[2] * b[2]; };
    if (sc.boundary == MER_BOUNDARY_SPHERE) {
        const double d[3] = {sc.sph_center[0] - O[0], sc.sph_center[1] - O[1], sc.sph_center[2] - O[2]};
        const double a = std::min(1.0, std::max(-1.0, dot3(d, U) / dot3(U, U))), b = std::min(1.0, std::max(-1.0, dot3(d, V) / dot3(V, V)));
        double d2 = 0;
        for (int i = 0; i < 3; i++) { const double e = O[i] + a * U[i] + b * V[i] - sc.sph_center[i]; d2 += e * e; }
        return d2 < (double) sc.sph_radius * sc.sph_radius;
    }
    double c[3], h[3];
    for (int i = 0; i < 3; i++) { c[i] = 0.5 * ((double) sc.bmin[i] + sc.bmax[i]) - O[i]; h[i] = 0.5 * ((double) sc.bmax[i] - sc.bmin[i]); }
    const double N[3] = {U[1] * V[2] - U[2] * V[1], U[2] * V[0] - U[0] * V[2], U[0] * V[1] - U[1] * V[0]};
    double axes[13][3];
    int na = 0;
    for (int i = 0; i < 3; i++) { axes[na][0] = axes[na][1] = axes[na][2] = 0; axes[na][i] = 1; na++; }
    for (const double *w : {U, V, N}) { for (int i = 0; i < 3; i++) axes[na][i] = w[i]; na++; }
    for (int i = 0; i < 3; i++)
        for (const double *w : {U, V}) {
            const double e[3] = {i == 0 ? 1.0 : 0.0, i == 1 ? 1.0 : 0.0, i == 2 ? 1.0 : 0.0};
            axes[na][0] = e[1] * w[2] - e[2] * w[1]; axes[na][1] = e[2] * w[0] - e[0] * w[2]; axes[na][2] = e[0] * w[1] - e[1] * w[0]; na++;
        }
    for (int k = 0; k < na; k++) {
        const double *L = axes[k];
        const double rBox = h[0] * std::fabs(L[0]) + h[1] * std::fabs(L[1]) + h[2] * std::fabs(L[2]);
        const double rRect = std::fabs(dot3(U, L)) + std::fabs(dot3(V, L));
        if (std::fabs(dot3(c, L)) > rBox + rRect) return false;           // separated (touching counts as meeting: the cube is closed)
    }
    return true;
}
// the rectangle lies outside the (convex) medium shape: the exact test, or the legacy area_* fields' five probes (corners and centre).  The
// probes test the box for every boundary value but the sphere, as they always did: an unknown value is refused by its own message later
static bool rect_outside(const mer_scene_desc &sc, const double M[3][4], bool exact) {
    if (exact) return !rect_meets_shape(sc, M);
    for (int k = 0; k < 5; k++) {
        const float lx = k == 4 ? 0.0f : (k & 1 ? 1.0f : -1.0f), ly = k == 4 ? 0.0f : (k & 2 ? 1.0f : -1.0f);
        const float q[3] = {(float) (M[0][0] * lx + M[0][1] * ly + M[0][3]), (float) (M[1][0] * lx + M[1][1] * ly + M[1][3]), (float) (M[2][0] * lx + M[2][1] * ly + M[2][3])};
        if (sc.boundary == MER_BOUNDARY_SPHERE ? point_in_sphere(sc, q) : point_in_box(sc, q)) return false;
    }
    return true;
}

// the disk O + a U + b V, a^2 + b^2 <= 1, lies outside the medium shape.  Sphere boundary: the disk's point closest to the centre (the
// centre's projection onto the plane, pulled back to the rim) lies outside -- exact.  Cube: the disk's circumscribed square passes the
// rectangle / box test -- conservative: a disk whose square cuts the cube with a corner the disk does not reach is refused too.
static bool disk_outside(const mer_scene_desc &sc, const double M[3][4]) {
    if (sc.boundary != MER_BOUNDARY_SPHERE) return !rect_meets_shape(sc, M);
    const double d[3] = {sc.sph_center[0] - M[0][3], sc.sph_center[1] - M[1][3], sc.sph_center[2] - M[2][3]};
    double a = (d[0] * M[0][0] + d[1] * M[1][0] + d[2] * M[2][0]) / col_dot(M, 0, 0), b = (d[0] * M[0][1] + d[1] * M[1][1] + d[2] * M[2][1]) / col_dot(M, 1, 1);
    const double r = std::sqrt(a * a + b * b);
    if (r > 1) { a /= r; b /= r; }
    double d2 = 0;
    for (int i = 0; i < 3; i++) { const double e = M[i][0] * a + M[i][1] * b - d[i]; d2 += e * e; }
    return !(d2 < (double) sc.sph_radius * sc.sph_radius);
}
// the sphere (centre = column 3 of M, radius R) is clear of the medium shape: apart from it (centre distance > R + r', or distance from the
// centre to the box > R), or -- a flipped sphere only -- around it (centre distance + r' < R, or the farthest corner of the box closer than R)
static bool sphere_clear(const mer_scene_desc &sc, const double M[3][4], double R, bool flipped) {
    const double c[3] = {M[0][3], M[1][3], M[2][3]};
    double nearest2 = 0, farthest2 = 0;
    if (sc.boundary == MER_BOUNDARY_SPHERE) {
        double d2 = 0; for (int i = 0; i < 3; i++) d2 += (c[i] - sc.sph_center[i]) * (c[i] - sc.sph_center[i]);
        const double d = std::sqrt(d2);
        return d > R + sc.sph_radius || (flipped && d + sc.sph_radius < R);
    }
    for (int i = 0; i < 3; i++) {
        const double lo = sc.bmin[i], hi = sc.bmax[i], out = std::max(std::max(lo - c[i], c[i] - hi), 0.0), far = std::max(std::fabs(c[i] - lo), std::fabs(c[i] - hi));
        nearest2 += out * out; farthest2 += far * far;
    }
    return nearest2 > R * R || (flipped && farthest2 < R * R);
}

// emitter `spot` (src/emitters/spot.cpp:68-95): the cone record of its point-table slot, in float as the reference derives it (degToRad in
// float, util.h:293; std::cos of the float angle).  The z row of the inverse linear part is computed in double and rounded.  Returns an
// error message or nullptr.
static const char *spot_derive(const mer_emitter &e, DSpot &s) {
    const float cdeg = e.cutoff_angle_deg, bdeg = e.beam_width_deg;
    if (!std::isfinite(cdeg) || !std::isfinite(bdeg) || cdeg < 0 || bdeg < 0) return "spot emitter: cutoffAngle and beamWidth must be finite and non-negative";
    if (cdeg > 180) return "spot emitter: cutoffAngle must not exceed 180 degrees";
    if (bdeg > cdeg) return "spot emitter: beamWidth must not exceed cutoffAngle (Assert(m_cutoffAngle >= m_beamWidth))";
    for (int i = 0; i < 12; i++) if (!std::isfinite(e.to_world[i])) return "spot emitter: 'toWorld' must be finite";
    double M[3][3], inv[3][3];
    linear3(e.to_world, M);
    const double det = inverse3(M, inv);
    if (!(std::fabs(det) > 0) || !std::isfinite(det)) return "spot emitter: 'toWorld' is singular";
    for (int i = 0; i < 3; i++) s.z[i] = (float) inv[2][i];
    const float beam = (float) (bdeg * (M_PI / 180.0f)), cutoff = (float) (cdeg * (M_PI / 180.0f));
    s.cos_beam = std::cos(beam); s.cos_cutoff = std::cos(cutoff);
    s.cutoff = cutoff; s.inv_width = 1.0f / (cutoff - beam);
    s.pad = 0;
    return nullptr;
}

// is the linear part of a row-major 3x4 matrix a rotation (M M^T = 1 within tol, det > 0)?  Transform::hasScale's question (transform.cpp)
static bool is_rotation(const float m[12], double tol) {
    for (int i = 0; i < 12; i++) if (!std::isfinite(m[i])) return false;
    double M[3][3];
    linear3(m, M);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const double d = M[r][0] * M[c][0] + M[r][1] * M[c][1] + M[r][2] * M[c][2] - (r == c ? 1.0 : 0.0);
            if (!(std::fabs(d) <= tol)) return false;
        }
    return det3(M) > 0;
}
// emitter `collimated` (src/emitters/collimated.cpp:58-66,115-124): the record of its point-table slot -- z = the beam's direction
// toWorld(0,0,1), both cosines -2 (falloff 1, as a point emitter's) and pad = 1, which marks the slot as a beam for the light tracer.
static const char *collimated_derive(const mer_emitter &e, DSpot &s) {
    for (int i = 0; i < 12; i++) if (!std::isfinite(e.to_world[i])) return "collimated emitter: 'toWorld' must be finite";
    if (!is_rotation(e.to_world, 1e-4)) return "Scale factors in the emitter-to-world transformation are not allowed!";      // collimated.cpp:63-65
    const double dx = e.to_world[2], dy = e.to_world[6], dz = e.to_world[10], len = std::sqrt(dx * dx + dy * dy + dz * dz);
    s.z[0] = (float) (dx / len); s.z[1] = (float) (dy / len); s.z[2] = (float) (dz / len);
    s.cos_cutoff = s.cos_beam = -2.0f; s.cutoff = 0; s.inv_width = 0; s.pad = 1.0f;
    return nullptr;
}

// emitter `envmap`: its record from the uploaded map and the entry's toWorld (a rotation within 1e-5; the translation is ignored -- a direction
// does not see it) and scale.  Returns an error message or nullptr.
static const char *envmap_derive(mer_context *ctx, const mer_emitter &e, DEnvMap &E) {
    auto it = ctx->envmaps.find(e.envmap);
    if (it == ctx->envmaps.end()) return "envmap emitter: unknown or destroyed envmap handle (mer_envmap_upload)";
    if (!std::isfinite(e.env_scale) || !(e.env_scale >= 0)) return "envmap emitter: 'scale' must be finite and non-negative";
    for (int i = 0; i < 12; i++) if (!std::isfinite(e.to_world[i])) return "envmap emitter: 'toWorld' must be finite";
    double M[3][3], inv[3][3];
    linear3(e.to_world, M);
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const double d = M[r][0] * M[c][0] + M[r][1] * M[c][1] + M[r][2] * M[c][2] - (r == c ? 1.0 : 0.0);
            if (std::fabs(d) > 1e-5) return "envmap emitter: the linear part of 'toWorld' must be a rotation (within 1e-5)";
        }
    if (!(inverse3(M, inv) > 0)) return "envmap emitter: the linear part of 'toWorld' must be a rotation (within 1e-5)";
    const EnvMap &m = it->second;
    const unsigned char *b = m.dev.as<const unsigned char>();
    E = DEnvMap{};
    E.texels = (const uint2 *) b; E.cdf_cols = (const float *) (b + m.off_cols); E.cdf_rows = (const float *) (b + m.off_rows);
    E.row_weights = (const float *) (b + m.off_weights);
    E.chk = ctx->chk;
    E.w = m.w; E.h = m.h; E.norm = m.norm; E.scale = e.env_scale;
    // trafo.inverse() of a rotation: its inverse matrix (in double, rounded), the rotation itself for the sampled direction (envmap.cpp:382, 537)
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) { E.w2l[3 * r + c] = (float) inv[r][c]; E.l2w[3 * r + c] = (float) M[r][c]; }
    E.pix[0] = (float) (2 * M_PI / m.w); E.pix[1] = (float) (M_PI / m.h);           // m_pixelSize (:312)
    return nullptr;
}

// One point-table record, with its cone (spot; NULL = a point emitter, falloff 1).  `at` prefixes the messages of a list entry; the
// legacy point_* fields pass list = false and are validated as they always were (a NaN intensity passes).
static int add_point(mer_context *ctx, const mer_scene_desc &sc, Emitters &em, const float pos[3], const float I[3], const DSpot *cone, double weight,
                     bool list, const std::string &at) {
    // Three preserved variants of one refusal: every kind refuses a negative intensity; a list entry also refuses a NaN one, a list point
    // a non-finite position and a spot a non-finite intensity (its position was checked with toWorld); the legacy fields test the sign only.
    for (int i = 0; i < 3; i++) {
        const bool negative = I[i] < 0;
        const bool list_nan = list && std::isnan(I[i]);
        const bool list_point_position = list && !cone && !std::isfinite(pos[i]);
        const bool list_spot_infinite = list && cone && !std::isfinite(I[i]);
        if (negative || list_nan || list_point_position || list_spot_infinite) return fail(ctx, at + "emitter radiance / intensity must be non-negative");
    }
    if (refuse_inside_rough(ctx, sc, nullptr, pos, cone != nullptr, at)) return 1;
    DPoint E{};
    for (int i = 0; i < 3; i++) { E.pos[i] = pos[i]; E.Ie[i] = I[i]; }
    DSpot none{}; none.cos_cutoff = none.cos_beam = -2.0f;
    em.tab.points[em.n_point] = E; em.tab.spots[em.n_point] = cone ? *cone : none; em.wp[em.n_point++] = weight;
    em.any_spot = em.any_spot || cone;
    return 0;
}
// One area-emitter record on a shape (AREA_RECT / AREA_DISK / AREA_SPHERE).  The legacy area_* fields (a rectangle, list = false) keep their
// five-probe outside test and no test of the radiance's sign.
static int add_rect(mer_context *ctx, const mer_scene_desc &sc, Emitters &em, int shape, const float to_world[12], const float radiance[3], double weight, bool list,
                    const std::string &at) {
    if (sc.rif_mode != MER_RIF_CONST) return fail(ctx, at + "the area emitter is built for straight rays (rif_mode = CONST)");
    if (sc.boundary_bsdf != MER_BSDF_NULL || sc.boundary == MER_BOUNDARY_SDF) return fail(ctx, at + "the area emitter needs an index-matched cube / sphere boundary");
    for (int i = 0; i < 3; i++) if (list && !(radiance[i] >= 0)) return fail(ctx, at + "emitter radiance / intensity must be non-negative");
    for (int i = 0; i < 12; i++) if (shape != AREA_RECT && !std::isfinite(to_world[i])) return fail(ctx, at + "area emitter: 'toWorld' must be finite");
    DRect R{}; double M[3][4];
    R.flip = 1.0f;
    if (const char *err = shape == AREA_SPHERE ? sphere_derive(to_world, R, M) : shape == AREA_DISK ? disk_derive(to_world, R, M) : rect_derive(to_world, R, M))
        return fail(ctx, at + err);
    if (shape == AREA_SPHERE) {
        if (!sphere_clear(sc, M, R.radius, R.flip < 0))
            return fail(ctx, at + "the area emitter's sphere must be clear of the medium shape (apart from it, or with inward normals around it)");
    } else if (shape == AREA_DISK) {
        if (!disk_outside(sc, M)) return fail(ctx, at + "the area emitter's disk must lie outside the medium shape");
    } else if (!rect_outside(sc, M, list)) return fail(ctx, at + "the area emitter's rectangle must lie outside the medium shape");
    for (int i = 0; i < 3; i++) R.L[i] = R.Le[i] = radiance[i];
    em.tab.rects[em.n_rect] = R; em.wr[em.n_rect++] = weight;
    return 0;
}
// selection pdf = weight / sum and CDF of one kind's records; the sample of record k is divided by its pdf on the host (intensity / pdf,
// radiance / pdf)
template <typename Rec> static void selection_cdf(Rec *rec, const double *w, int n, float (Rec::*value)[3]) {
    double sum = 0, cum = 0;
    for (int k = 0; k < n; ++k) sum += w[k];
    for (int k = 0; k < n; ++k) {
        cum += w[k];
        rec[k].pdf = (float) (w[k] / sum); rec[k].cdf = k + 1 == n ? 1.0f : (float) (cum / sum);
        for (int i = 0; i < 3; i++) (rec[k].*value)[i] = (rec[k].*value)[i] / rec[k].pdf;
    }
}

// mer_scene_desc.emitters -> records: each entry checked as the single emitter of its kind is, the rectangles by the exact outside test
static int emitter_list(mer_context *ctx, const mer_scene_desc &sc, Emitters &em) {
    if (sc.n_emitters < 0 || sc.n_emitters > MER_MAX_EMITTERS) return fail(ctx, "emitter list: at most " + std::to_string(MER_MAX_EMITTERS) + " entries (MER_MAX_EMITTERS)");
    if (!sc.emitters) return fail(ctx, "emitter list: n_emitters > 0 but no entries");
    if (em.n_point || em.n_rect) return fail(ctx, "emitter list: the point_* / area_* emitter fields must be zero when n_emitters > 0");
    for (int j = 0; j < sc.n_emitters; ++j) {
        const mer_emitter &e = sc.emitters[j];
        const std::string at = "emitter list, entry " + std::to_string(j) + ": ";
        if (!(e.sampling_weight > 0) || !std::isfinite(e.sampling_weight)) return fail(ctx, at + "samplingWeight must be positive");
        if (e.type == MER_EMITTER_POINT) {
            if (add_point(ctx, sc, em, e.position, e.intensity, nullptr, e.sampling_weight, true, at)) return 1;
        } else if (e.type == MER_EMITTER_SPOT) {      // a point emitter at toWorld's origin with a cone: it joins the point table
            DSpot cone{};
            if (const char *err = spot_derive(e, cone)) return fail(ctx, at + err);
            const float pos[3] = {e.to_world[3], e.to_world[7], e.to_world[11]};
            if (add_point(ctx, sc, em, pos, e.intensity, &cone, e.sampling_weight, true, at)) return 1;
        } else if (e.type == MER_EMITTER_COLLIMATED) {   // a beam: a point-table slot whose cone record carries the direction (DSpot::pad = 1); light tracing only
            if (sc.integrator != MER_INTEGRATOR_PTRACER)
                return fail(ctx, at + "a collimated emitter is a delta in position and direction: no camera path can sample it (it would render black); use integrator = ptracer");
            DSpot beam{};
            if (const char *err = collimated_derive(e, beam)) return fail(ctx, at + err);
            const float pos[3] = {e.to_world[3], e.to_world[7], e.to_world[11]};
            if (add_point(ctx, sc, em, pos, e.intensity, &beam, e.sampling_weight, true, at)) return 1;
        } else if (e.type == MER_EMITTER_AREA || e.type == MER_EMITTER_AREA_DISK || e.type == MER_EMITTER_AREA_SPHERE) {   // one kind, one CDF, in list order
            const int shape = e.type == MER_EMITTER_AREA_SPHERE ? AREA_SPHERE : e.type == MER_EMITTER_AREA_DISK ? AREA_DISK : AREA_RECT;
            if (add_rect(ctx, sc, em, shape, e.to_world, e.radiance, e.sampling_weight, true, at)) return 1;
        } else if (e.type == MER_EMITTER_ENVMAP) {    // the environment: its own kind, one at most, sampled at every collision (selection probability 1)
            if (em.has_env || sc.env_radiance[0] != 0 || sc.env_radiance[1] != 0 || sc.env_radiance[2] != 0)
                return fail(ctx, at + "The scene may only contain one environment emitter (an envmap entry excludes a second one and a non-zero env_radiance)");
            if (const char *err = envmap_derive(ctx, e, em.tab.env)) return fail(ctx, at + err);
            em.has_env = true;
        } else return fail(ctx, at + "unknown emitter type");
    }
    if (em.n_rect)
        for (int k = 0; k < em.n_point; ++k)
            if (!point_in_shape(sc, em.tab.points[k].pos))
                return fail(ctx, "emitter list: a point or spot emitter outside the medium shape cannot be combined with an area emitter (point samples are not tested against rectangles)");
    return 0;
}

// ---- the steps of make_params, in its order -----------------------------------------------------------------------------------------

// integrator = ptracer: what the light tracer (mer_ptracer.hpp) is built for; everything else is refused here, from the scene's fields alone,
// before any step touches the device
static int ptracer_scope(mer_context *ctx, const mer_scene_desc &sc) {
    const std::string at = "ptracer: ";
    if (sc.sensor != MER_SENSOR_PERSPECTIVE) return fail(ctx, at + "light paths are connected to the perspective sensor only (orthographic, thinlens and telecentric are not built)");
    if (!is_rotation(sc.cam_to_world, 1e-4)) return fail(ctx, at + "cam_to_world must be a rigid transformation (its inverse is taken as the transpose)");
    if (sc.env_radiance[0] != 0 || sc.env_radiance[1] != 0 || sc.env_radiance[2] != 0) return fail(ctx, at + "a constant environment (env_radiance) is not built for light tracing");
    if (sc.emission[0] != 0 || sc.emission[1] != 0 || sc.emission[2] != 0) return fail(ctx, at + "medium emission is not built for light tracing");
    if (sc.point_intensity[0] != 0 || sc.point_intensity[1] != 0 || sc.point_intensity[2] != 0 || sc.area_radiance[0] != 0 || sc.area_radiance[1] != 0 || sc.area_radiance[2] != 0)
        return fail(ctx, at + "emitters are given as list entries (mer_scene_desc.emitters); the point_* / area_* fields must be zero");
    if (sc.n_emitters <= 0 || !sc.emitters) return fail(ctx, at + "the scene has no emitter (list entries of kind point, spot or collimated)");
    for (int j = 0; j < sc.n_emitters && j < MER_MAX_EMITTERS; ++j) {
        const mer_emitter &e = sc.emitters[j];
        const std::string ej = at + "emitter list, entry " + std::to_string(j) + ": ";
        if (e.type == MER_EMITTER_ENVMAP) return fail(ctx, ej + "an envmap emitter is not built for light tracing");
        if (e.type == MER_EMITTER_AREA || e.type == MER_EMITTER_AREA_DISK || e.type == MER_EMITTER_AREA_SPHERE) return fail(ctx, ej + "area emitters are not built for light tracing");
        if (e.type == MER_EMITTER_SPOT && !is_rotation(e.to_world, 1e-4)) return fail(ctx, ej + "a spot emitter's 'toWorld' must be free of scale for light tracing (its cone is sampled about the z axis)");
    }
    if (sc.boundary == MER_BOUNDARY_SDF) return fail(ctx, at + "the signed-distance boundary is not built for light tracing (cube or sphere)");
    if (sc.boundary_bsdf != MER_BSDF_NULL) return fail(ctx, at + "dielectric boundaries are not built for light tracing (the index-matched null boundary)");
    if (sc.sigma_mode == MER_SIGMA_GRID && sc.method == MER_METHOD_SIMPSON) return fail(ctx, at + "method = simpson is not built for light tracing (woodcock)");
    if (sc.stepper != MER_STEP_VERLET && sc.stepper != MER_STEP_RK4 && sc.rif_mode != MER_RIF_CONST) return fail(ctx, at + "unknown stepper (verlet, rk4)");
    if (sc.rif_mode == MER_RIF_TRILINEAR) {
        auto it = ctx->volumes.find(sc.rif);
        if (it != ctx->volumes.end() && it->second.cell8)
            return fail(ctx, at + "the index field must be uploaded in the dense layout (the CELL8 / BRICK record layouts are not built for light tracing)");
    }
    return 0;
}

static int integrator(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    if (sc.width <= 0 || sc.height <= 0) return fail(ctx, "film: width/height must be positive");
    if (sc.rr_depth <= 0) return fail(ctx, "'rrDepth' must be set to a value greater than zero!");                 // integrator.cpp:217
    if (sc.max_depth <= 0 && sc.max_depth != -1)
        return fail(ctx, "'maxDepth' must be set to -1 (infinite) or a value greater than zero!");                  // integrator.cpp:220
    if (sc.phase == MER_PHASE_HG && (sc.g >= 1 || sc.g <= -1))
        return fail(ctx, "The asymmetry parameter must lie in the interval (-1, 1)!");                              // hg.cpp:52-53
    if (sc.integrator != MER_INTEGRATOR_VOLPATH && sc.integrator != MER_INTEGRATOR_PTRACER) return fail(ctx, "integrator: unknown integrator (volpath, ptracer)");
    if (sc.integrator_reserved != 0) return fail(ctx, "integrator: integrator_reserved must be 0");
    if (sc.integrator == MER_INTEGRATOR_PTRACER) return ptracer_scope(ctx, sc);
    return 0;
}

// heterogeneous medium: the density grid and the simpson method's step
static int density_grid(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    if (sc.sigma_mode == MER_SIGMA_GRID) {
        auto it = ctx->volumes.find(sc.density);
        if (it == ctx->volumes.end()) return fail(ctx, "No density specified!");                                    // heterogeneous.cpp:229-230
        if (it->second.desc.channels != 1) return fail(ctx, "density volume must support float lookups");           // :270
        if (it->second.layout == MER_LAYOUT_BRICK27 || it->second.layout == MER_LAYOUT_BRICK125) return fail(ctx, "the BRICK layouts are for the refractive-index field only");
        fill_dgrid(ctx, it->second, P.density);
        if (!(sc.density_scale > 0)) return fail(ctx, "heterogeneous medium: 'scale' must be positive");
        // m_maxDensity = m_scale * getMaximumFloatValue() (= 1.0 for gridvolume): heterogeneous.cpp:239-242
        P.inv_max_density = 1.0f / (sc.density_scale * 1.0f);
        if (sc.method != MER_METHOD_WOODCOCK && sc.method != MER_METHOD_SIMPSON) return fail(ctx, "Unsupported integration method!");    // heterogeneous.cpp:195-202
        if (sc.method == MER_METHOD_SIMPSON) {
            if (sc.rif_mode != MER_RIF_CONST) return fail(ctx, "method = simpson belongs to the heterogeneous medium (straight rays)");
            auto step_of = [](const mer_grid_desc &g) {                      // gridvolume.cpp:196-198
                float s = std::numeric_limits<float>::infinity();
                for (int i = 0; i < 3; i++) s = std::min(s, 0.5f * (g.aabb_max[i] - g.aabb_min[i]) / (float) (g.res[i] - 1));
                return s;
            };
            float h = sc.het_stepsize;                                      // heterogeneous.cpp:245-257
            if (h == 0) {
                h = step_of(it->second.desc);
                if (sc.albedo_mode == MER_ALBEDO_GRID) { auto ia = ctx->volumes.find(sc.albedo_grid); if (ia != ctx->volumes.end()) h = std::min(h, step_of(ia->second.desc)); }
            }
            if (!(h > 0) || !std::isfinite(h))
                return fail(ctx, "Unable to infer a suitable step size for deterministic integration, please specify one manually using the 'stepSize' parameter.");
            P.het_step = h;
            P.sc.tr_estimator = MER_TR_RATIO;        // one walk per transmittance query (the estimator choice is the Woodcock method's)
        }
    }
    return 0;
}
static int albedo_grid(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    if (sc.albedo_mode == MER_ALBEDO_GRID) {
        auto it = ctx->volumes.find(sc.albedo_grid);
        if (it == ctx->volumes.end()) return fail(ctx, "No albedo specified!");                                     // heterogeneous.cpp:231-232
        if (it->second.desc.channels != 3) return fail(ctx, "albedo volume must support spectrum lookups");
        fill_dgrid(ctx, it->second, P.albedo, false);
    }
    return 0;
}
// heterogeneousrefractive: the analytic acoustic field, or the RIF grid with its index-range refusals
static int rif_grid(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    if (sc.rif_mode == MER_RIF_ACOUSTIC) {
        // acousticrifvolume: analytic, no grid (src/volume/acousticrifvolume.cpp:101-106)
        if (!(sc.stepsize > 0)) return fail(ctx, "heterogeneousrefractive: 'stepsize' must be positive");
        if (!(sc.ac_k_r > 0) || !(sc.ac_n_o > 0) || sc.ac_mode < 0 || !std::isfinite(sc.ac_n_max)) return fail(ctx, "acousticrifvolume: n_o and k_r = 2 pi freq / speed must be positive, mode non-negative");
        std::memset(&P.rif, 0, sizeof(P.rif));
        P.rif.ac_n_o = sc.ac_n_o; P.rif.ac_n_max = sc.ac_n_max; P.rif.ac_k_r = sc.ac_k_r; P.rif.ac_mode = sc.ac_mode;
        P.rif.res[0] = P.rif.res[1] = P.rif.res[2] = 2;
    } else if (sc.rif_mode != MER_RIF_CONST) {
        if (sc.rif_mode != MER_RIF_TRILINEAR && sc.rif_mode != MER_RIF_BSPLINE3) return fail(ctx, "unknown rif_mode");
        auto it = ctx->volumes.find(sc.rif);
        if (it == ctx->volumes.end()) return fail(ctx, "No RIF specified!");                                        // heterogeneousrefractive.cpp:368-369
        if (it->second.desc.channels != 1 || it->second.desc.dtype != MER_VOL_F32)
            return fail(ctx, "RIF volume must be a 1-channel float32 grid");
        if (sc.rif_mode == MER_RIF_BSPLINE3 && !it->second.coeff)
            return fail(ctx, "RIF volume has no spline coefficients (call mer_volume_build_spline)");
        if (!(sc.stepsize > 0)) return fail(ctx, "heterogeneousrefractive: 'stepsize' must be positive");
        fill_dgrid(ctx, it->second, P.rif);
        // the fetch index (z * res_y + y) * res_x + x is formed with 24-bit multiplies (v_mul_u32_u24)
        if ((int64_t) P.rif.res[1] * P.rif.res[2] > ((int64_t) 1 << 24) || P.rif.res[0] > (1 << 24))
            return fail(ctx, "RIF volume: res_y * res_z must not exceed 2^24 (index arithmetic of the trilinear fetch)");
        if ((int64_t) P.rif.res[0] * P.rif.res[1] * P.rif.res[2] >= ((int64_t) 1 << 31))
            return fail(ctx, "RIF volume: more than 2^31 nodes (the cell id of the trilinear fetch is a 32-bit integer)");
        if (P.rif.affine && it->second.cell8)
            return fail(ctx, "RIF volume with a toWorld transform: upload it in the dense layout (the CELL8 / BRICK record layouts carry no transform)");
        if (sc.rif_mode == MER_RIF_BSPLINE3) {
            for (int i = 0; i < 3; i++) if (P.rif.res[i] < 5) return fail(ctx, "splinevolume needs at least 5 nodes per axis");
            // the medium must lie inside the spline-safe box (gate: heterogeneousrefractive.cpp:461-466)
        }
    }
    return 0;
}

// sigmaA / sigmaS / sigmaT and mediumSamplingWeight
static int coefficients(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    for (int i = 0; i < 3; i++) {
        if (sc.sigma_a[i] < 0 || sc.sigma_s[i] < 0) return fail(ctx, "sigmaA / sigmaS must be non-negative");
    }
    P.sigA = f3(sc.sigma_a[0], sc.sigma_a[1], sc.sigma_a[2]);
    P.sigS = f3(sc.sigma_s[0], sc.sigma_s[1], sc.sigma_s[2]);
    P.sigT = f3(sc.sigma_a[0] + sc.sigma_s[0], sc.sigma_a[1] + sc.sigma_s[1], sc.sigma_a[2] + sc.sigma_s[2]);
    const float sT[3] = {P.sigT.x, P.sigT.y, P.sigT.z}, sS[3] = {P.sigS.x, P.sigS.y, P.sigS.z};
    // mediumSamplingWeight: homogeneous.cpp:172-190 == heterogeneousrefractive.cpp:239-255
    float w = sc.medium_sampling_weight;
    if (w == -1) {
        for (int i = 0; i < 3; ++i) {
            const float albedo = sS[i] / sT[i];
            if (albedo > w && sT[i] != 0) w = albedo;
        }
        if (w > 0) w = std::max(w, 0.5f);
    }
    P.medium_sampling_weight = w;
    return 0;
}
// the distance-sampling strategy: single / manual densities, the maximum strategy's tables
static int sampling_strategy(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    const float sT[3] = {P.sigT.x, P.sigT.y, P.sigT.z};
    P.sampling_density = 0;
    if (sc.strategy == MER_STRATEGY_SINGLE) {
        int channel = 0; float smallest = std::numeric_limits<float>::infinity();
        for (int i = 0; i < 3; ++i) if (sT[i] < smallest) { smallest = sT[i]; channel = i; }
        if (sc.channel >= 0) { if (sc.channel > 2) return fail(ctx, "channel out of range"); channel = sc.channel; }
        P.sampling_density = sT[channel];
    } else if (sc.strategy == MER_STRATEGY_MANUAL) {
        P.sampling_density = sc.sampling_density;
    } else if (sc.strategy == MER_STRATEGY_MAXIMUM) {
        // MaxExpDist's constructor (src/medium/maxexp.h:30-58), in the reference's float arithmetic
        MaxExp &m = P.maxexp;
        for (int i = 0; i < 3; i++) m.sigmaT[i] = sT[i];
        std::sort(m.sigmaT, m.sigmaT + 3, std::greater<float>());
        m.cdf[0] = 0;
        for (int i = 0; i < 3; ++i) {
            if (i > 0 && m.sigmaT[i] == m.sigmaT[i - 1]) return fail(ctx, "Internal error: sigmaT must vary across channels");
            if (!(m.sigmaT[i] > 0)) return fail(ctx, "strategy maximum: sigmaT must be positive in every channel");
            const float lower = (i == 0) ? -1 : -std::pow((m.sigmaT[i] / m.sigmaT[i - 1]), -m.sigmaT[i] / (m.sigmaT[i] - m.sigmaT[i - 1]));
            const float upper = (i == 2) ? 0 : -std::pow((m.sigmaT[i + 1] / m.sigmaT[i]), -m.sigmaT[i] / (m.sigmaT[i + 1] - m.sigmaT[i]));
            m.cdf[i + 1] = m.cdf[i] + (upper - lower);
            m.intervalStart[i] = (i == 0) ? 0 : std::log(m.sigmaT[i] / m.sigmaT[i - 1]) / (m.sigmaT[i] - m.sigmaT[i - 1]);
        }
        m.normalization = m.cdf[3]; m.invNormalization = 1 / m.normalization;
        for (int i = 0; i < 4; ++i) m.cdf[i] *= m.invNormalization;
    } else if (sc.strategy != MER_STRATEGY_BALANCE) {
        return fail(ctx, "Specified an unknown sampling strategy");                                                 // homogeneous.cpp:226
    }
    if (sc.sigma_mode == MER_SIGMA_HOMOGENEOUS && !(sT[0] > 0 && sT[1] > 0 && sT[2] > 0) && sc.strategy == MER_STRATEGY_BALANCE)
        return fail(ctx, "homogeneous medium: sigmaT must be positive in every channel for the balance strategy");
    return 0;
}

static int sensor(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    P.aspect = (float) sc.width / (float) sc.height;
    P.cot_half_fov = 1.0f / std::tan((sc.fov_x_deg / 2.0f) * (MER_PI / 180.0f));
    for (int i = 0; i < 3; i++) P.par_dir[i] = 0.0f;
    P.sensor_pad[0] = 0.0f;
    P.lens_radius = P.lens_focus = 0.0f;
    if (sc.sensor < MER_SENSOR_PERSPECTIVE || sc.sensor > MER_SENSOR_TELECENTRIC) return fail(ctx, "sensor: unknown sensor kind (perspective, orthographic, thinlens, telecentric)");
    if (sc.sensor_reserved != 0) return fail(ctx, "sensor: sensor_reserved must be 0");
    if (sc.sensor != MER_SENSOR_PERSPECTIVE) {
        // what the sensors' constructors / configure() derive from toWorld (orthographic.cpp:133, telecentric.cpp:140-147), in float
        const float *m = sc.cam_to_world;
        bool finite = true;
        for (int i = 0; i < 12; i++) finite = finite && std::isfinite(m[i]);
        double M[3][3];
        linear3(m, M);
        if (!finite || !(std::fabs(det3(M)) > 1e-12)) return fail(ctx, "sensor: cam_to_world is singular");
        float len[3];
        for (int c = 0; c < 3; c++) len[c] = std::sqrt(m[c] * m[c] + m[4 + c] * m[4 + c] + m[8 + c] * m[8 + c]);
        for (int r = 0; r < 3; r++) P.par_dir[r] = m[4 * r + 2] / len[2];
        if (sc.sensor != MER_SENSOR_ORTHOGRAPHIC) {
            if (!(sc.aperture_radius >= 0) || !std::isfinite(sc.aperture_radius)) return fail(ctx, "sensor: aperture_radius must be finite and non-negative");
            if (!(sc.focus_distance > 0) || !std::isfinite(sc.focus_distance)) return fail(ctx, "sensor: focus_distance must be finite and positive");
            const bool tele = sc.sensor == MER_SENSOR_TELECENTRIC;
            P.lens_radius = tele ? sc.aperture_radius / len[0] : sc.aperture_radius;
            P.lens_focus = tele ? sc.focus_distance / len[2] : sc.focus_distance;
        }
    }
    P.inv_res_x = 1.0f / sc.width; P.inv_res_y = 1.0f / sc.height;
    return 0;
}

static int reconstruction_filter(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    if (sc.rfilter != MER_FILTER_BOX && sc.rfilter != MER_FILTER_GAUSSIAN) return fail(ctx, "unknown reconstruction filter");
    if (!(sc.rfilter_param > 0)) return fail(ctx, "reconstruction filter radius/stddev must be positive");
    // the table goes to device memory once per (kind, parameter); no kernel of this context is in flight here (renders and leaf calls return synchronised)
    float fv[33];
    filter_table(sc.rfilter, sc.rfilter_param, fv, P.fradius, P.fscale);
    if (ctx->ftable.reserve(ctx, sizeof(fv))) return 1;
    if (ctx->ftable_kind != sc.rfilter || ctx->ftable_param != sc.rfilter_param) {
        HIP_CHECK(ctx, hipMemcpy(ctx->ftable.p, fv, sizeof(fv), hipMemcpyHostToDevice));
        ctx->ftable_kind = sc.rfilter; ctx->ftable_param = sc.rfilter_param;
    }
    P.ftable = ctx->ftable.as<float>();
    if (P.fradius > 7.0f) return fail(ctx, "reconstruction filter radius too large");
    return 0;
}

static int boundary_bsdf(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    if (sc.boundary_bsdf != MER_BSDF_NULL && sc.boundary_bsdf != MER_BSDF_HDIELECTRIC && sc.boundary_bsdf != MER_BSDF_HROUGHDIELECTRIC)
        return fail(ctx, "boundary BSDF must be null, hdielectric or hroughdielectric");
    if (sc.boundary_bsdf == MER_BSDF_HROUGHDIELECTRIC && check_rough(ctx, &sc)) return 1;
    return 0;
}

// The legacy point_* / area_* fields are a list of at most one point and one rectangle with selection weight 1 (pdf = cdf = 1); then
// mer_scene_desc.emitters; then every kind's selection pdf and CDF.
static int emitters(mer_context *ctx, const mer_scene_desc &sc, Params &P, Emitters &em) {
    if (sc.point_intensity[0] != 0 || sc.point_intensity[1] != 0 || sc.point_intensity[2] != 0)
        if (add_point(ctx, sc, em, sc.point_position, sc.point_intensity, nullptr, 1.0, false, "")) return 1;
    if (sc.area_radiance[0] != 0 || sc.area_radiance[1] != 0 || sc.area_radiance[2] != 0)
        if (add_rect(ctx, sc, em, AREA_RECT, sc.area_to_world, sc.area_radiance, 1.0, false, "")) return 1;
    if (sc.n_emitters != 0 && emitter_list(ctx, sc, em)) return 1;
    if (!em.any_spot) std::memset(em.tab.spots, 0, sizeof(em.tab.spots));     // point-only scenes carry no cone table: the kernels skip the falloff
    selection_cdf(em.tab.points, em.wp, em.n_point, &DPoint::Ie);
    selection_cdf(em.tab.rects, em.wr, em.n_rect, &DRect::Le);
    return 0;
}

static int film(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    if (film_frames(ctx, &sc, P.frames)) return 1;
    P.film_ch = P.frames * 3 + 2;
    P.mod_phase = (float) (sc.mod_phase_deg * M_PI / 180);                                                   // pathlengthsampler.cpp:15
    return 0;
}

// the medium shape: cube, sphere or signed-distance grid (and, with the grid known, the rough boundary's test of the point table)
static int boundary_shape(mer_context *ctx, const mer_scene_desc &sc, Params &P, const Emitters &em, bool allow_sdf) {
    if (sc.boundary == MER_BOUNDARY_AABB) {
        for (int i = 0; i < 3; i++) if (!(sc.bmin[i] < sc.bmax[i])) return fail(ctx, "medium shape: empty bounding box");
    } else if (sc.boundary == MER_BOUNDARY_SPHERE) {
        if (!(sc.sph_radius > 0)) return fail(ctx, "medium shape: sphere radius must be positive");
    } else if (sc.boundary == MER_BOUNDARY_SDF) {
        if (!allow_sdf) return fail(ctx, "the signed-distance boundary is known to mer_render only (leaf entry points: cube / sphere)");
        auto it = ctx->volumes.find(sc.sdf);
        if (it == ctx->volumes.end()) return fail(ctx, "heterogeneousrefractive: no sdf volume (boundary = sdf)");
        if (it->second.desc.channels != 1 || it->second.desc.dtype != MER_VOL_F32) return fail(ctx, "heterogeneousrefractive: the sdf must be a 1-channel float32 grid");
        if (it->second.layout == MER_LAYOUT_BRICK27 || it->second.layout == MER_LAYOUT_BRICK125) return fail(ctx, "the BRICK layouts are for the refractive-index field only");
        fill_dgrid(ctx, it->second, P.sdf);
        float d2 = 0; for (int i = 0; i < 3; i++) d2 += (P.sdf.bmax[i] - P.sdf.bmin[i]) * (P.sdf.bmax[i] - P.sdf.bmin[i]);
        P.sdf_eps = 1e-4f * std::sqrt(d2);
        for (int k = 0; k < em.n_point; ++k) if (refuse_inside_rough(ctx, sc, &P.sdf, em.tab.points[k].pos, false, "")) return 1;
    } else return fail(ctx, "unknown medium boundary");
    return 0;
}

static int aggressive_tracing(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    if (sc.aggressive_tracing) {
        if (sc.boundary != MER_BOUNDARY_SDF) return fail(ctx, "aggressivetracing needs the signed-distance boundary (the medium's sdf volume)");
        if (sc.rif_mode == MER_RIF_CONST) return fail(ctx, "aggressivetracing is a property of curved-ray tracing (heterogeneousrefractive)");
        if (!(sc.sdf_max_error >= 0)) return fail(ctx, "aggressivetracing: sdf_max_error must be non-negative");
    }
    return 0;
}

// emitter `constant`: the last of the scene's checks
static int constant_environment(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    for (int i = 0; i < 3; i++) if (sc.env_radiance[i] < 0) return fail(ctx, "emitter radiance / intensity must be non-negative");
    return 0;
}

// The emitter table goes to device memory when it changes; no kernel of this context is in flight here (renders and leaf calls return
// synchronised).
static int emitter_upload(mer_context *ctx, const mer_scene_desc &sc, Params &P, const Emitters &em) {
    if (ctx->etab.reserve(ctx, sizeof(EmitterTable))) return 1;
    if (!ctx->etab_valid || std::memcmp(&ctx->etab_host, &em.tab, sizeof(EmitterTable)) != 0) {
        HIP_CHECK(ctx, hipMemcpy(ctx->etab.p, &em.tab, sizeof(EmitterTable), hipMemcpyHostToDevice));
        ctx->etab_host = em.tab; ctx->etab_valid = true;
    }
    P.n_point = em.n_point; P.n_rect = em.n_rect;
    EmitterTable *etab = ctx->etab.as<EmitterTable>();
    P.points = etab->points; P.rects = etab->rects;
    P.has_spot = em.any_spot ? 1 : 0;              // the kernels find the cones (spot_table)
    P.has_envmap = em.has_env ? 1 : 0;             // and the envmap's record (envmap_rec) behind the rectangles: EmitterTable
    return 0;
}

static int context_pointers(mer_context *ctx, const mer_scene_desc &sc, Params &P) {
    P.counters = ctx->counters.as<unsigned long long>();
    P.work_counter = P.counters + MER_C_COUNT * MER_COUNTER_REPLICAS;
    P.chk = ctx->chk;
    P.dbg_pixel = (int32_t) ctx->opt.debug_pixel;
    return 0;
}

// Validate the scene the way the reference plugins' constructors / configure() do, and flatten it.  The order of the steps is the order of
// the checks: which message a doubly invalid scene gets is behaviour.  A new plugin parameter goes into the step of its plugin.
int make_params(mer_context *ctx, const mer_scene_desc *scene, Params &P, bool allow_sdf, bool *point_outside) {
    const mer_scene_desc &sc = *scene;
    std::memset(&P, 0, sizeof(P));
    P.sc = sc;
    Emitters em;
    std::memset(&em.tab, 0, sizeof(em.tab));
    if (integrator(ctx, sc, P) || density_grid(ctx, sc, P) || albedo_grid(ctx, sc, P) || rif_grid(ctx, sc, P) ||
        coefficients(ctx, sc, P) || sampling_strategy(ctx, sc, P) || sensor(ctx, sc, P) || reconstruction_filter(ctx, sc, P) ||
        boundary_bsdf(ctx, sc, P) || emitters(ctx, sc, P, em) || film(ctx, sc, P) || boundary_shape(ctx, sc, P, em, allow_sdf) ||
        aggressive_tracing(ctx, sc, P) || constant_environment(ctx, sc, P) || emitter_upload(ctx, sc, P, em) || context_pointers(ctx, sc, P))
        return 1;
    // curved rays reach a point emitter outside the (cube / sphere) shape through the boundary (Connector::path_lengths, cross = true)
    if (point_outside) {
        *point_outside = false;
        for (int k = 0; k < em.n_point; ++k) if (sc.boundary != MER_BOUNDARY_SDF && !point_in_shape(sc, em.tab.points[k].pos)) *point_outside = true;
    }
    return 0;
}

}  // namespace mer
