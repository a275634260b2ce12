// edge_geom.hip — distances of GIVEN edges as a differentiable function of the atomic positions (forces at fixed topology).
// No reference counterpart: the reference builds its graphs once on the host (process.py:258-305) and has no force path.
//
//   mdl_edge_geometry_fwd   per edge (src -> tgt, batch-global node ids of packed structures): dist = fp32 of the fp64
//                           minimum-image |p_tgt - p_src + shift| and the unit vector u of that displacement.  The image is
//                           chosen by the code graph_build.hip runs (graph_geom.inc: reduced cell, completed basis, rint wrap,
//                           +-1 images), contraction off in both files: dist is bitwise the builder's for the same pair.
//                           Self loops and coincident atoms (d = 0) get u = 0.
//   mdl_edge_geometry_bwd   dpos[n] = sum_{e: tgt(e) = n} dd_e u_e - sum_{e: src(e) = n} dd_e u_e, one lane per atom walking its
//                           row of the by-target CSR and its row of the by-source CSR: no atomics, the same bits on every run.
//                           The cell is held fixed (no stress).
#include "mdl_common.h"

#pragma clang fp contract(off)

namespace mdl {
namespace {

#include "graph_geom.inc"

__global__ __launch_bounds__(256) void edge_geom_fwd_kernel(const double* __restrict__ pos, const int64_t* __restrict__ node_ptr,
                                                            const GraphGeom* __restrict__ geom, int64_t N, int64_t G,
                                                            const int32_t* __restrict__ src, const int32_t* __restrict__ tgt, int64_t E,
                                                            float* __restrict__ dist, float* __restrict__ u) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= E) return;
    const int64_t i = src[e], j = tgt[e];
    float d = 0.0f, ux = 0.0f, uy = 0.0f, uz = 0.0f;
    if (i >= 0 && i < N && j >= 0 && j < N) {
        int64_t lo_g = 0, hi_g = G;                            // graph of the source: the last g with node_ptr[g] <= i
        while (hi_g - lo_g > 1) {
            const int64_t mid = (lo_g + hi_g) >> 1;
            if (node_ptr[mid] <= i) lo_g = mid;
            else hi_g = mid;
        }
        const GraphGeom* gm = geom + lo_g;
        const double dx = pos[j * 3 + 0] - pos[i * 3 + 0], dy = pos[j * 3 + 1] - pos[i * 3 + 1], dz = pos[j * 3 + 2] - pos[i * 3 + 2];
        double v[3] = {0.0, 0.0, 0.0};
        const double r = sqrt(min_image_r2<true>(gm, gm->nimg, gm->pbc, dx, dy, dz, v));
        d = (float)r;
        if (r > 0.0) {
            ux = (float)(v[0] / r);
            uy = (float)(v[1] / r);
            uz = (float)(v[2] / r);
        }
    }
    dist[e] = d;
    u[e * 3 + 0] = ux;
    u[e * 3 + 1] = uy;
    u[e * 3 + 2] = uz;
}

// row n of a CSR over the edges: slots [rowptr[n], rowptr[n + 1]), edge id of a slot = eid[slot] (null: the slot itself)
__device__ __forceinline__ void edge_row_sum(const float* __restrict__ dd, const float* __restrict__ u, const int32_t* __restrict__ rowptr,
                                             const int32_t* __restrict__ eid, int64_t n, int64_t E, double* acc) {
    for (int64_t q = rowptr[n]; q < rowptr[n + 1]; ++q) {
        const int64_t e = eid ? (int64_t)eid[q] : q;
        if (e < 0 || e >= E) continue;
        const double g = (double)dd[e];
        acc[0] += g * (double)u[e * 3 + 0];
        acc[1] += g * (double)u[e * 3 + 1];
        acc[2] += g * (double)u[e * 3 + 2];
    }
}

__global__ __launch_bounds__(256) void edge_geom_bwd_kernel(const float* __restrict__ dd, const float* __restrict__ u,
                                                            const int32_t* __restrict__ rowptr_t, const int32_t* __restrict__ eid_t,
                                                            const int32_t* __restrict__ rowptr_s, const int32_t* __restrict__ eid_s,
                                                            int64_t N, int64_t E, float* __restrict__ dpos) {
    const int64_t n = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= N) return;
    double at[3] = {0.0, 0.0, 0.0}, as[3] = {0.0, 0.0, 0.0};
    edge_row_sum(dd, u, rowptr_t, eid_t, n, E, at);
    edge_row_sum(dd, u, rowptr_s, eid_s, n, E, as);
    dpos[n * 3 + 0] = (float)(at[0] - as[0]);
    dpos[n * 3 + 1] = (float)(at[1] - as[1]);
    dpos[n * 3 + 2] = (float)(at[2] - as[2]);
}

}  // namespace
}  // namespace mdl

extern "C" size_t mdl_edge_geometry_workspace_bytes(int64_t G) {
    return G < 1 ? 0 : (size_t)G * sizeof(mdl::GraphGeom);
}

extern "C" int mdl_edge_geometry_fwd(const double* pos, const int64_t* node_ptr, const double* cell, const int32_t* pbc, int64_t N,
                                     int64_t G, const int32_t* src, const int32_t* tgt, int64_t E, float* dist, float* u,
                                     void* workspace, size_t workspace_bytes, mdlStream_t stream) {
    using namespace mdl;
    MDL_REQUIRE(N >= 1 && G >= 1 && E >= 0, MDL_E_ARG, "mdl_edge_geometry_fwd: need N >= 1 atoms, G >= 1 graphs, E >= 0 (got N=%lld G=%lld E=%lld)",
                (long long)N, (long long)G, (long long)E);
    MDL_REQUIRE(N < (1ll << 31), MDL_E_UNSUPP, "mdl_edge_geometry_fwd: N=%lld overflows the int32 node ids", (long long)N);
    if (E == 0) return MDL_OK;
    MDL_REQUIRE(pos && node_ptr && cell && pbc && src && tgt && dist && u && workspace, MDL_E_ARG, "mdl_edge_geometry_fwd: null pointer");
    MDL_REQUIRE(workspace_bytes >= (size_t)G * sizeof(GraphGeom), MDL_E_ARG, "mdl_edge_geometry_fwd: workspace of %zu bytes, the launch needs %zu",
                workspace_bytes, (size_t)G * sizeof(GraphGeom));
    MDL_REQUIRE(((uintptr_t)workspace & 7) == 0, MDL_E_ARG, "mdl_edge_geometry_fwd: workspace not 8-byte aligned");
    GraphGeom* geom = (GraphGeom*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(graph_geom_kernel, dim3((unsigned)cdiv(G, 64)), dim3(64), 0, st, cell, pbc, G, geom);
    hipLaunchKernelGGL(edge_geom_fwd_kernel, dim3((unsigned)cdiv(E, 256)), dim3(256), 0, st, pos, node_ptr, geom, N, G, src, tgt, E, dist, u);
    return check_launch("mdl_edge_geometry_fwd");
}

extern "C" int mdl_edge_geometry_bwd(const float* dd, const float* u, const int32_t* rowptr_t, const int32_t* eid_t,
                                     const int32_t* rowptr_s, const int32_t* eid_s, int64_t N, int64_t E, float* dpos,
                                     mdlStream_t stream) {
    using namespace mdl;
    MDL_REQUIRE(N >= 0 && E >= 0, MDL_E_ARG, "mdl_edge_geometry_bwd: bad N=%lld E=%lld", (long long)N, (long long)E);
    if (N == 0) return MDL_OK;
    MDL_REQUIRE(rowptr_t && rowptr_s && dpos && (E == 0 || (dd && u)), MDL_E_ARG, "mdl_edge_geometry_bwd: null pointer");
    hipLaunchKernelGGL(edge_geom_bwd_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, (hipStream_t)stream, dd, u, rowptr_t, eid_t,
                       rowptr_s, eid_s, N, E, dpos);
    return check_launch("mdl_edge_geometry_bwd");
}
