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
//                           The cell is held fixed here; its derivative is the reduction below.
//   mdl_edge_strain_grad    out[g] = sum_{e in graph g} dd_e d_e u_e (x) u_e, the derivative of the energy w.r.t. a homogeneous
//                           strain of structure g at fixed neighbour lists and images (d|v|/d eps_ab = v_a v_b / |v|).  The edges
//                           of a graph are one contiguous slot range of the by-target CSR; one workgroup per (graph, slice), six
//                           fp64 sums per lane, wave64 shuffles, then the waves through LDS in wave order: no atomics, the same
//                           bits on every run.
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

constexpr int STRAIN_THREADS = 256;
constexpr int STRAIN_WAVES = STRAIN_THREADS / WAVE;
constexpr int STRAIN_MAX_SLICES = 65536;

// slices per graph from E and G alone (nothing is read back): one workgroup per graph once the graphs fill the device or
// are small, else enough slices of >= 2048 slots to put about 1024 workgroups on it
inline int64_t strain_slices(int64_t G, int64_t E, int64_t slices) {
    if (slices > 0) return slices;
    if (G < 1 || G >= 1024 || E / G <= 4096) return 1;
    const int64_t by_dev = cdiv(1024, G), by_len = cdiv(E / G, 2048);
    const int64_t s = by_dev < by_len ? by_dev : by_len;
    return s > 256 ? 256 : s;
}

// component k of the six sums (xx, xy, xz, yy, yz, zz) -> its one or two places in the row-major 3x3
__device__ __forceinline__ void strain_store(float* __restrict__ o, int k, double v) {
    const int first[6] = {0, 1, 2, 4, 5, 8}, second[6] = {0, 3, 6, 4, 7, 8};
    const float f = (float)v;
    o[first[k]] = f;
    o[second[k]] = f;
}

__global__ __launch_bounds__(STRAIN_THREADS) void edge_strain_kernel(const float* __restrict__ dd, const float* __restrict__ dist,
                                                                     const float* __restrict__ u, const int32_t* __restrict__ rowptr_t,
                                                                     const int32_t* __restrict__ eid_t, const int64_t* __restrict__ node_ptr,
                                                                     int64_t N, int64_t E, int S, float* __restrict__ out,
                                                                     double* __restrict__ part) {
    __shared__ double red[STRAIN_WAVES][6];
    const int64_t g = blockIdx.x / S, s = blockIdx.x % S;
    int64_t n0 = node_ptr[g], n1 = node_ptr[g + 1];
    n0 = n0 < 0 ? 0 : (n0 > N ? N : n0);
    n1 = n1 < n0 ? n0 : (n1 > N ? N : n1);
    int64_t q0 = rowptr_t[n0], q1 = rowptr_t[n1];              // the graph's slots: contiguous in the by-target CSR
    q0 = q0 < 0 ? 0 : (q0 > E ? E : q0);
    q1 = q1 < q0 ? q0 : (q1 > E ? E : q1);
    const int64_t share = (q1 - q0 + S - 1) / S;
    const int64_t a = q0 + s * share, b = a + share < q1 ? a + share : q1;
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t q = a + threadIdx.x; q < b; q += STRAIN_THREADS) {
        const int64_t e = eid_t ? (int64_t)eid_t[q] : q;
        if (e < 0 || e >= E) continue;
        const double w = (double)dd[e] * (double)dist[e];
        const double ux = (double)u[e * 3 + 0], uy = (double)u[e * 3 + 1], uz = (double)u[e * 3 + 2];
        const double wx = w * ux, wy = w * uy;
        acc[0] += wx * ux;
        acc[1] += wx * uy;
        acc[2] += wx * uz;
        acc[3] += wy * uy;
        acc[4] += wy * uz;
        acc[5] += w * uz * uz;
    }
#pragma unroll
    for (int k = 0; k < 6; ++k)
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) acc[k] += __shfl_down(acc[k], off, WAVE);
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < 6; ++k) red[wave][k] = acc[k];
    __syncthreads();
    if (threadIdx.x < 6) {
        const int k = threadIdx.x;
        double v = red[0][k];
#pragma unroll
        for (int w = 1; w < STRAIN_WAVES; ++w) v += red[w][k];
        if (S == 1) strain_store(out + g * 9, k, v);
        else part[((int64_t)blockIdx.x) * 6 + k] = v;
    }
}

// S > 1: out[g] from the partial sums part [G, S, 6], added in slice order; one lane per (graph, component)
__global__ __launch_bounds__(256) void edge_strain_finish_kernel(const double* __restrict__ part, int64_t G, int S, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= G * 6) return;
    const int64_t g = t / 6;
    const int k = (int)(t % 6);
    double v = 0.0;
    for (int s = 0; s < S; ++s) v += part[(g * S + s) * 6 + k];
    strain_store(out + g * 9, k, v);
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

extern "C" size_t mdl_edge_strain_grad_workspace_bytes(int64_t G, int64_t E, int32_t slices) {
    const int64_t S = mdl::strain_slices(G, E, slices);
    return G < 1 || S <= 1 ? 0 : (size_t)G * (size_t)S * 6 * sizeof(double);
}

extern "C" int mdl_edge_strain_grad(const float* dd, const float* dist, const float* u, const int32_t* rowptr_t, const int32_t* eid_t,
                                    const int64_t* node_ptr, int64_t N, int64_t G, int64_t E, int32_t slices, float* out,
                                    void* workspace, size_t workspace_bytes, mdlStream_t stream) {
    using namespace mdl;
    MDL_REQUIRE(N >= 0 && G >= 0 && E >= 0, MDL_E_ARG, "mdl_edge_strain_grad: bad N=%lld G=%lld E=%lld", (long long)N, (long long)G, (long long)E);
    MDL_REQUIRE(slices >= 0 && slices <= STRAIN_MAX_SLICES, MDL_E_ARG, "mdl_edge_strain_grad: slices=%d outside [0, %d] (0: chosen from E and G)",
                (int)slices, STRAIN_MAX_SLICES);
    if (G == 0) return MDL_OK;
    MDL_REQUIRE(E < (1ll << 31), MDL_E_UNSUPP, "mdl_edge_strain_grad: E=%lld overflows the int32 edge slots", (long long)E);
    MDL_REQUIRE(rowptr_t && node_ptr && out && (E == 0 || (dd && dist && u)), MDL_E_ARG, "mdl_edge_strain_grad: null pointer");
    const int64_t S = strain_slices(G, E, slices);
    MDL_REQUIRE(G * S < (1ll << 31), MDL_E_UNSUPP, "mdl_edge_strain_grad: G=%lld graphs x %lld slices overflow the grid", (long long)G, (long long)S);
    hipStream_t st = (hipStream_t)stream;
    double* part = nullptr;
    if (S > 1) {
        const size_t need = (size_t)G * (size_t)S * 6 * sizeof(double);
        MDL_REQUIRE(workspace && workspace_bytes >= need, MDL_E_ARG, "mdl_edge_strain_grad: workspace of %zu bytes, the launch needs %zu",
                    workspace ? workspace_bytes : (size_t)0, need);
        MDL_REQUIRE(((uintptr_t)workspace & 7) == 0, MDL_E_ARG, "mdl_edge_strain_grad: workspace not 8-byte aligned");
        part = (double*)workspace;
    }
    hipLaunchKernelGGL(edge_strain_kernel, dim3((unsigned)(G * S)), dim3(STRAIN_THREADS), 0, st, dd, dist, u, rowptr_t, eid_t, node_ptr, N, E,
                       (int)S, out, part);
    if (S > 1)
        hipLaunchKernelGGL(edge_strain_finish_kernel, dim3((unsigned)cdiv(G * 6, 256)), dim3(256), 0, st, part, G, (int)S, out);
    return check_launch("mdl_edge_strain_grad");
}
