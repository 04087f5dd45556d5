// mer_sdf_build.hip -- signed-distance grid of a triangle mesh (mer_sdf_from_mesh, include/mer.h): a dense all-pairs pass, every grid
// node against every triangle.  Per node: the unsigned distance is the minimum over the triangles of the point-triangle distance
// (closest point by Voronoi regions, Ericson, Real-Time Collision Detection 5.1.5), the sign comes from the generalized winding number
// (Van Oosterom-Strackee solid angles): inside iff |w| >= 0.5, output negative inside.  A translation unit of its own: no render
// kernel is compiled from here.
//
// One thread per node (x fastest, the VOL payload order); the triangle loop is wave-uniform.  The triangles are processed in chunks,
// one launch per (node range, triangle chunk), with the per-node running state (min d^2, sum of the atan2 terms) kept in device
// memory between the launches, so that no launch runs long.  Every node adds its triangles in index order in float32 whatever the
// chunking, so the result is bit-identical for every chunk size.
#include "mer_internal.hpp"

namespace mer {

enum { CHK_SDF_NODE = 32, CHK_SDF_TRI = 33 };      // bounds-check kinds of this unit (mer_device.hpp numbers the others from 1)

// a triangle on the device: 3 x float4 (xyz of a vertex, w unused), so that a vertex is one 16-byte load
__device__ __forceinline__ f3 sdf_sub(float4 v, f3 p) { return f3(v.x - p.x, v.y - p.y, v.z - p.z); }

// one (node, triangle) pair; a, b, c = the triangle's vertices minus the node
__device__ __forceinline__ void sdf_pair(f3 a, f3 b, f3 c, float &d2min, float &wsum) {
    // closest point of the triangle to the origin as a + ab * s + ac * t; the regions are tested in Ericson's order
    const f3 ab = b - a, ac = c - a;
    const float d1 = -dot(ab, a), d2 = -dot(ac, a);
    const float d3 = -dot(ab, b), d4 = -dot(ac, b);
    const float d5 = -dot(ab, c), d6 = -dot(ac, c);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4;
    float ns, nt, den;
    if (d1 <= 0.0f && d2 <= 0.0f) { ns = 0.0f; nt = 0.0f; den = 1.0f; }                                   // vertex a
    else if (d3 >= 0.0f && d4 <= d3) { ns = 1.0f; nt = 0.0f; den = 1.0f; }                                // vertex b
    else if (vc <= 0.0f && d1 >= 0.0f && d3 <= 0.0f) { ns = d1; nt = 0.0f; den = d1 - d3; }               // edge ab
    else if (d6 >= 0.0f && d5 <= d6) { ns = 0.0f; nt = 1.0f; den = 1.0f; }                                // vertex c
    else if (vb <= 0.0f && d2 >= 0.0f && d6 <= 0.0f) { ns = 0.0f; nt = d2; den = d2 - d6; }               // edge ac
    else if (va <= 0.0f && (d4 - d3) >= 0.0f && (d5 - d6) >= 0.0f) { ns = d5 - d6; nt = d4 - d3; den = (d4 - d3) + (d5 - d6); }   // edge bc
    else { ns = vb; nt = vc; den = (va + vb) + vc; }                                                      // face
    const float s = ns / den, t = nt / den;
    const f3 q = (a + ab * s) + ac * t;
    d2min = fminf(d2min, dot(q, q));
    // solid angle of the triangle seen from the node, over 2: atan2(a . (b x c), |a||b||c| + (a.b)|c| + (b.c)|a| + (c.a)|b|)
    const float la = sqrtf(dot(a, a)), lb = sqrtf(dot(b, b)), lc = sqrtf(dot(c, c));
    const float num = dot(a, cross(b, c));
    const float dn = ((la * lb * lc + dot(a, b) * lc) + dot(b, c) * la) + dot(c, a) * lb;
    wsum = wsum + atan2f(num, dn);
}

#define MER_SDF_BLOCK 256

// nodes [node0, node1), triangles [t0, t1) of the n_tri in `tri`; state d2s / ws per node, initialised here when t0 == 0.  Every lane reads
// the triangle at the same, wave-uniform address: the compiler turns these into scalar loads, one per wave.  (Staging 256 triangles at a
// time in LDS and broadcasting them measured the same pair rate, 2.52e11 against 2.54e11 pairs/s at 256^3 x 20480, and cost two barriers per
// tile: not kept.)
__global__ __launch_bounds__(MER_SDF_BLOCK) void sdf_accum_kernel(SdfGridArgs g, const float4 *__restrict__ tri, uint32_t n_tri, uint32_t t0, uint32_t t1,
                                                                  uint64_t node0, uint64_t node1, float *__restrict__ d2s, float *__restrict__ ws) {
    const uint64_t n = node0 + (uint64_t) blockIdx.x * MER_SDF_BLOCK + threadIdx.x;
    if (n >= node1) return;
    const uint32_t ix = (uint32_t) (n % (uint64_t) g.res[0]);
    const uint64_t r = n / (uint64_t) g.res[0];
    const uint32_t iy = (uint32_t) (r % (uint64_t) g.res[1]), iz = (uint32_t) (r / (uint64_t) g.res[1]);
    const f3 p(g.lo[0] + (float) ix * g.step[0], g.lo[1] + (float) iy * g.step[1], g.lo[2] + (float) iz * g.step[2]);
    const uint64_t at = MER_CHK(g.chk, CHK_SDF_NODE, n, g.n_nodes);
    float d2min = t0 == 0 ? INFINITY : d2s[at], wsum = t0 == 0 ? 0.0f : ws[at];
    for (uint32_t t = t0; t < t1; t++) {
        const float4 *v = tri + MER_CHK(g.chk, CHK_SDF_TRI, (uint64_t) t * 3u, (uint64_t) n_tri * 3u - 2u);
        sdf_pair(sdf_sub(v[0], p), sdf_sub(v[1], p), sdf_sub(v[2], p), d2min, wsum);
    }
    d2s[at] = d2min; ws[at] = wsum;
}

// in place: d2s becomes the signed distance, ws the winding number
__global__ __launch_bounds__(MER_SDF_BLOCK) void sdf_finish_kernel(SdfGridArgs g, float *__restrict__ d2s, float *__restrict__ ws) {
    const uint64_t n = (uint64_t) blockIdx.x * MER_SDF_BLOCK + threadIdx.x;
    if (n >= g.n_nodes) return;
    const uint64_t at = MER_CHK(g.chk, CHK_SDF_NODE, n, g.n_nodes);
    const float d = sqrtf(d2s[at]);
    const float w = ws[at] * 0.15915494309189535f;           // sum of atan2 terms x 2 / (4 pi)
    d2s[at] = fabsf(w) >= 0.5f ? -d : d;
    ws[at] = w;
}

int sdf_build(mer_context *ctx, const mer_grid_desc *d, const float *tri12_host, int64_t n_tri, int32_t max_tri_per_launch, DeviceBuffer &sdf, DeviceBuffer &winding) {
    SdfGridArgs g;
    g.n_nodes = (uint64_t) d->res[0] * (uint64_t) d->res[1] * (uint64_t) d->res[2];
    for (int a = 0; a < 3; a++) {
        g.res[a] = d->res[a]; g.lo[a] = d->aabb_min[a];
        g.step[a] = (d->aabb_max[a] - d->aabb_min[a]) / (float) (d->res[a] - 1);
    }
    g.chk = ctx->chk;
    const uint32_t chunk = max_tri_per_launch > 0 ? (uint32_t) max_tri_per_launch : (uint32_t) MER_SDF_DEFAULT_CHUNK;
    DeviceBuffer tri;
    if (tri.alloc(ctx, (size_t) n_tri * 48) || sdf.alloc(ctx, g.n_nodes * 4) || winding.alloc(ctx, g.n_nodes * 4)) return 1;
    float *d2s = sdf.as<float>(), *ws = winding.as<float>();
    HIP_CHECK(ctx, hipMemcpyAsync(tri.p, tri12_host, (size_t) n_tri * 48, hipMemcpyHostToDevice, ctx->stream));
    // triangle chunks outermost: a node range meets its chunks in index order
    for (uint32_t t0 = 0; t0 < (uint32_t) n_tri; t0 += chunk) {
        const uint32_t t1 = (uint32_t) std::min<int64_t>(n_tri, (int64_t) t0 + chunk);
        for (uint64_t n0 = 0; n0 < g.n_nodes; n0 += MER_SDF_NODES_PER_LAUNCH) {
            const uint64_t n1 = std::min<uint64_t>(g.n_nodes, n0 + MER_SDF_NODES_PER_LAUNCH);
            const dim3 grid(nblocks((int64_t) (n1 - n0), MER_SDF_BLOCK));
            hipLaunchKernelGGL(sdf_accum_kernel, grid, dim3(MER_SDF_BLOCK), 0, ctx->stream, g, tri.as<const float4>(), (uint32_t) n_tri, t0, t1, n0, n1, d2s, ws);
            HIP_CHECK(ctx, hipGetLastError());
        }
    }
    hipLaunchKernelGGL(sdf_finish_kernel, dim3(nblocks((int64_t) g.n_nodes, MER_SDF_BLOCK)), dim3(MER_SDF_BLOCK), 0, ctx->stream, g, d2s, ws);
    HIP_CHECK(ctx, hipGetLastError());
    HIP_CHECK(ctx, hipStreamSynchronize(ctx->stream));          // before `tri` goes
    return 0;
}

}  // namespace mer
