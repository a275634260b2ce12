// graph_build.hip — crystal graphs on the device: the per-structure graph rule of
// the reference's matdeeplearn/process/process.py:258-305,385-388,540-559,594-605 as the host builder
// matdeeplearn_amd/process/graph.py restates it, for a whole batch of structures in one call.
//
// Per structure with n atoms (rows i and columns j over all n atoms):
//   1. Distance.  d[i,j] is the fp64 minimum-image distance of graph.distance_matrix: the periodic cell vectors are
//      reduced (reduce_cell), the basis is completed for 1-D / 2-D periodicity, the fractional difference of
//      p_j - p_i is wrapped with rint, r^2 is minimised over the +-1 images of the periodic axes, then sqrt.
//      Non-periodic structures take the plain difference.  ONE value per atom pair (its minimum image): not a
//      multi-image radius graph, so no cell list.
//   2. Selection.  Row i keeps column j when the ordinal rank of (d[i,j], j) in the row (ascending, ties to the lower
//      column) is <= k + 1 and d[i,j] <= radius (threshold_sort), then drops exact zeros of the fp32 value
//      (edges_from_trimmed): the diagonal and coincident atoms use up rank slots but give no edge.
//   3. Edges.  Every kept (i, j) is an edge source i -> target j, weight float32(d); plus one self loop per node,
//      weight 0.
//   4. Order.  CSR by target (graph.sort_by_target, stable): the in-edges of target t with ascending sources, then
//      the self loop of t.
//   5. out_deg[i] = kept edges of row i + 1 (the one-hot degree feature of process.py:594-605 counts the loop).
//
// Kernels (all deterministic: bitwise the same output run to run):
//   graph_geom_kernel   one lane per structure: reduced cell, completed basis, its inverse, the image shifts (fp64).
//   graph_rows_kernel   one wave per source row: lanes stream over the columns 64 at a time; the candidates within
//                       the radius of a chunk are bitonic-sorted on (d, j) and merged into the row's running k smallest
//                       (one key per lane).  The diagonal is left out of the selection: the k + 1 smallest keys with it
//                       hold the same non-zero entries as the k smallest without it (see graph_rows_kernel).  Kept
//                       entries take a slot in their target's in-edge list with an integer atomic.
//   graph_scan_*        exclusive scan of (in-degree + 1) over all nodes: the CSR row pointer, whose values at the
//                       first node of every graph are edge_ptr.
//   graph_place_kernel  every kept entry to rowptr[target] + slot.
//   graph_sort_kernel   one lane per target: its in-edges sorted by source (sources are distinct, so the atomic slot
//                       order is forgotten), the self loop last.
//
// Exactness: the distance arithmetic is evaluated in the operation order of graph.distance_matrix with FMA
// contraction off (the pragma below, and -ffp-contract=off in _build.FILE_FLAGS).  For a basis with one non-zero per
// row and column (orthorhombic cells, with any pbc) np.linalg.inv returns the correctly rounded reciprocals, and so
// does the special case below: orthorhombic and non-periodic distances are bitwise those of the host.  Other bases
// are inverted through the adjugate: the distances may differ from the host's in the last fp64 bits.
#include "mdl_common.h"

#pragma clang fp contract(off)

namespace mdl {
namespace {

constexpr int GB_MAX_K = 64;
constexpr int SCAN_TILE = 2048;                // 256 threads x 8 nodes
constexpr size_t WS_ALIGN = 256;

#include "graph_geom.inc"

__device__ __forceinline__ bool key_less(double a, int ja, double b, int jb) { return a < b || (a == b && ja < jb); }

// compare-exchange with lane ^ stride: keep the smaller key if keep_min, else the larger
__device__ __forceinline__ void cmpx(double& d, int& j, int stride, bool keep_min) {
    const double od = __shfl_xor(d, stride);
    const int oj = __shfl_xor(j, stride);
    const bool take = keep_min ? key_less(od, oj, d, j) : key_less(d, j, od, oj);
    if (take) {
        d = od;
        j = oj;
    }
}

// One wave per source row i.  Row i's keys are (d[i,j], j) for the columns within the radius.  The diagonal (0, i) is
// left out: if at most k keys precede it (coincident atoms j < i), the k + 1 smallest keys are it plus the k smallest of
// the others; if more do, the k + 1 smallest are all zeros and so are the k smallest of the others.  Either way the
// non-zero entries are those of the k smallest non-diagonal keys, which fit one per lane (k <= 64).
__global__ __launch_bounds__(256) void graph_rows_kernel(const double* __restrict__ pos, const int64_t* __restrict__ node_ptr,
                                                         const GraphGeom* __restrict__ geom, int64_t N, int64_t G, double radius,
                                                         int k, int32_t* __restrict__ nbr_tgt, int32_t* __restrict__ nbr_slot,
                                                         float* __restrict__ nbr_d, int32_t* __restrict__ row_base,
                                                         int32_t* __restrict__ in_cnt, int32_t* __restrict__ out_deg) {
    const int lane = threadIdx.x & 63;
    const int64_t i = (int64_t)blockIdx.x * (blockDim.x / WAVE) + (threadIdx.x >> 6);
    if (i >= N) return;
    // graph of row i: the last g with node_ptr[g] <= i (empty graphs before it are skipped); bounds clamped to [0, N]
    int64_t lo_g = 0, hi_g = G;
    while (hi_g - lo_g > 1) {
        const int64_t mid = (lo_g + hi_g) >> 1;
        if (node_ptr[mid] <= i) lo_g = mid;
        else hi_g = mid;
    }
    const int64_t g = lo_g;
    const int64_t start = min(max(node_ptr[g], (int64_t)0), N);
    const int64_t end = min(max(node_ptr[g + 1], start), N);
    const bool valid = i >= start && i < end;
    const int n = valid ? (int)(end - start) : 0;
    const int li = (int)(i - start);
    const double px = pos[i * 3 + 0], py = pos[i * 3 + 1], pz = pos[i * 3 + 2];
    const GraphGeom* gm = geom + g;
    const int nimg = valid ? gm->nimg : 0;
    const int mask = gm->pbc;

    double Ld = __builtin_inf();                              // running k smallest keys, ascending over the lanes
    int Lj = 0x7fffffff;
    for (int base = 0; base < n; base += WAVE) {
        const int j = base + lane;
        double cd = __builtin_inf();
        int cj = 0x7fffffff;
        if (j < n && j != li) {
            const int64_t gj = start + j;
            const double dx = pos[gj * 3 + 0] - px, dy = pos[gj * 3 + 1] - py, dz = pos[gj * 3 + 2] - pz;
            const double r2 = min_image_r2<false>(gm, nimg, mask, dx, dy, dz, nullptr);
            const double d = sqrt(r2);
            if (d <= radius) {
                cd = d;
                cj = j;
            }
        }
        // skip the chunk when none of its keys beats the current k-th smallest
        const double wd = __shfl(Ld, k - 1);
        const int wj = __shfl(Lj, k - 1);
        if (!__any(key_less(cd, cj, wd, wj))) continue;
        // bitonic sort of the chunk, ascending
        for (int size = 2; size <= WAVE; size <<= 1)
            for (int stride = size >> 1; stride > 0; stride >>= 1) cmpx(cd, cj, stride, ((lane & stride) == 0) == ((lane & size) == 0));
        // min(L ascending, chunk descending) holds the 64 smallest as a bitonic sequence; merge it ascending
        const double rd = __shfl(cd, WAVE - 1 - lane);
        const int rj = __shfl(cj, WAVE - 1 - lane);
        if (key_less(rd, rj, Ld, Lj)) {
            Ld = rd;
            Lj = rj;
        }
        for (int stride = WAVE / 2; stride > 0; stride >>= 1) cmpx(Ld, Lj, stride, (lane & stride) == 0);
    }
    const float df = (float)Ld;
    const bool keep = lane < k && Lj != 0x7fffffff && df != 0.0f;
    const int64_t e = i * k + lane;
    if (lane < k) {
        int32_t slot = 0;
        if (keep) slot = atomicAdd(in_cnt + start + Lj, 1);
        nbr_tgt[e] = keep ? (int32_t)(start + Lj) : -1;
        nbr_slot[e] = slot;
        nbr_d[e] = df;
    }
    const int kept = __popcll(__ballot(keep));
    if (lane == 0) {
        out_deg[i] = kept + 1;
        row_base[i] = (int32_t)start;
    }
}

// inclusive wave scan of 64-bit values
__device__ __forceinline__ int64_t wave_incl_scan(int64_t v, int lane) {
    for (int off = 1; off < WAVE; off <<= 1) {
        const int64_t t = __shfl_up(v, off);
        if (lane >= off) v += t;
    }
    return v;
}

// rowptr[t] = exclusive prefix of (in_cnt + 1) inside the 2048-node tile; tile_sum[b] = the tile's total
__global__ __launch_bounds__(256) void graph_scan_tiles_kernel(const int32_t* __restrict__ in_cnt, int64_t N,
                                                               int64_t* __restrict__ rowptr, int64_t* __restrict__ tile_sum) {
    __shared__ int64_t s_w[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t base = (int64_t)blockIdx.x * SCAN_TILE + threadIdx.x * 8;
    int64_t v[8], sum = 0;
    for (int q = 0; q < 8; ++q) {
        v[q] = sum;
        sum += base + q < N ? (int64_t)in_cnt[base + q] + 1 : 0;
    }
    const int64_t incl = wave_incl_scan(sum, lane);
    if (lane == WAVE - 1) s_w[w] = incl;
    __syncthreads();
    int64_t wpre = 0;
    for (int q = 0; q < w; ++q) wpre += s_w[q];
    const int64_t excl = wpre + incl - sum;
    for (int q = 0; q < 8; ++q)
        if (base + q < N) rowptr[base + q] = excl + v[q];
    if (threadIdx.x == 255) tile_sum[blockIdx.x] = wpre + incl;
}

// one workgroup: tile_sum -> exclusive tile offsets in place; rowptr[N] = total
__global__ __launch_bounds__(256) void graph_scan_top_kernel(int64_t* __restrict__ tile_sum, int64_t T, int64_t N,
                                                             int64_t* __restrict__ rowptr) {
    __shared__ int64_t s_w[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    int64_t carry = 0;
    for (int64_t b0 = 0; b0 < T; b0 += 256) {
        const int64_t b = b0 + threadIdx.x;
        const int64_t v = b < T ? tile_sum[b] : 0;
        const int64_t incl = wave_incl_scan(v, lane);
        if (lane == WAVE - 1) s_w[w] = incl;
        __syncthreads();
        int64_t wpre = 0, tot = 0;
        for (int q = 0; q < 4; ++q) {
            if (q < w) wpre += s_w[q];
            tot += s_w[q];
        }
        if (b < T) tile_sum[b] = carry + wpre + incl - v;
        carry += tot;
        __syncthreads();
    }
    if (threadIdx.x == 0) rowptr[N] = carry;
}

__global__ __launch_bounds__(256) void graph_scan_add_kernel(const int64_t* __restrict__ tile_off, int64_t N, int64_t* __restrict__ rowptr) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < N) rowptr[t] += tile_off[t / SCAN_TILE];
}

__global__ __launch_bounds__(256) void graph_place_kernel(const int32_t* __restrict__ nbr_tgt, const int32_t* __restrict__ nbr_slot,
                                                          const float* __restrict__ nbr_d, const int32_t* __restrict__ row_base,
                                                          const int64_t* __restrict__ rowptr, int64_t NK, int k,
                                                          int32_t* __restrict__ src, int32_t* __restrict__ tgt, float* __restrict__ dist) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= NK) return;
    const int32_t t = nbr_tgt[e];
    if (t < 0) return;
    const int64_t i = e / k;
    const int32_t base = row_base[i];
    const int64_t p = rowptr[t] + nbr_slot[e];
    src[p] = (int32_t)(i - base);
    tgt[p] = t - base;
    dist[p] = nbr_d[e];
}

// one lane per target: in-edges sorted by source (insertion sort: ~k entries), the self loop last
__global__ __launch_bounds__(256) void graph_sort_kernel(const int64_t* __restrict__ rowptr, const int32_t* __restrict__ row_base,
                                                         int64_t N, int32_t* __restrict__ src, int32_t* __restrict__ tgt,
                                                         float* __restrict__ dist) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= N) return;
    const int64_t b = rowptr[t], e = rowptr[t + 1] - 1;
    for (int64_t p = b + 1; p < e; ++p) {
        const int32_t s = src[p];
        const float d = dist[p];
        int64_t q = p - 1;
        while (q >= b && src[q] > s) {
            src[q + 1] = src[q];
            dist[q + 1] = dist[q];
            --q;
        }
        src[q + 1] = s;
        dist[q + 1] = d;
    }
    const int32_t lt = (int32_t)(t - row_base[t]);
    src[e] = lt;
    tgt[e] = lt;
    dist[e] = 0.0f;
}

__global__ __launch_bounds__(256) void graph_edge_ptr_kernel(const int64_t* __restrict__ node_ptr, const int64_t* __restrict__ rowptr,
                                                             int64_t G, int64_t N, int64_t* __restrict__ edge_ptr) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (g > G) return;
    edge_ptr[g] = rowptr[min(max(node_ptr[g], (int64_t)0), N)];
}

struct Layout {
    size_t geom, nbr_tgt, nbr_slot, nbr_d, row_base, in_cnt, rowptr, tiles, total;
};

size_t up(size_t v) { return (v + WS_ALIGN - 1) / WS_ALIGN * WS_ALIGN; }

Layout layout(int64_t N, int64_t G, int k) {
    Layout l;
    const size_t nk = (size_t)N * (size_t)k, T = (size_t)cdiv(N, SCAN_TILE);
    size_t o = 0;
    l.geom = o;     o += up((size_t)G * sizeof(GraphGeom));
    l.nbr_tgt = o;  o += up(nk * 4);
    l.nbr_slot = o; o += up(nk * 4);
    l.nbr_d = o;    o += up(nk * 4);
    l.row_base = o; o += up((size_t)N * 4);
    l.in_cnt = o;   o += up((size_t)N * 4);
    l.rowptr = o;   o += up((size_t)(N + 1) * 8);
    l.tiles = o;    o += up(T * 8);
    l.total = o;
    return l;
}

}  // namespace
}  // namespace mdl

extern "C" size_t mdl_graph_workspace_bytes(int64_t N, int64_t G, int max_neighbors) {
    if (N < 1 || G < 1 || max_neighbors < 1 || max_neighbors > mdl::GB_MAX_K) return 0;
    return mdl::layout(N, G, max_neighbors).total;
}

extern "C" int mdl_graph_build(const double* pos, const int64_t* node_ptr, const double* cell, const int32_t* pbc, int64_t N,
                               int64_t G, double radius, int max_neighbors, int64_t* edge_ptr, int32_t* src, int32_t* tgt,
                               float* dist, int32_t* out_deg, int64_t edge_capacity, void* workspace, size_t workspace_bytes,
                               mdlStream_t stream) {
    using namespace mdl;
    const int k = max_neighbors;
    MDL_REQUIRE(k >= 1 && k <= GB_MAX_K, MDL_E_UNSUPP, "mdl_graph_build: max_neighbors=%d outside the supported 1..%d", k, GB_MAX_K);
    MDL_REQUIRE(radius > 0.0, MDL_E_ARG, "mdl_graph_build: radius must be positive (got %g)", radius);
    MDL_REQUIRE(N >= 1 && G >= 1, MDL_E_ARG, "mdl_graph_build: need N >= 1 atoms and G >= 1 graphs (got N=%lld G=%lld)",
                (long long)N, (long long)G);
    MDL_REQUIRE(N * (int64_t)(k + 1) < (1ll << 31), MDL_E_UNSUPP, "mdl_graph_build: N*(k+1) = %lld edges overflow int32",
                (long long)(N * (k + 1)));
    MDL_REQUIRE(pos && node_ptr && cell && pbc && edge_ptr && src && tgt && dist && out_deg && workspace, MDL_E_ARG,
                "mdl_graph_build: null pointer");
    MDL_REQUIRE(edge_capacity >= N * (int64_t)(k + 1), MDL_E_ARG, "mdl_graph_build: edge capacity %lld < N*(k+1) = %lld",
                (long long)edge_capacity, (long long)(N * (k + 1)));
    const Layout l = layout(N, G, k);
    MDL_REQUIRE(workspace_bytes >= l.total, MDL_E_ARG, "mdl_graph_build: workspace of %zu bytes, the launch needs %zu",
                workspace_bytes, l.total);
    MDL_REQUIRE(((uintptr_t)workspace & (WS_ALIGN - 1)) == 0, MDL_E_ARG, "mdl_graph_build: workspace not %zu-byte aligned", WS_ALIGN);
    char* ws = (char*)workspace;
    GraphGeom* geom = (GraphGeom*)(ws + l.geom);
    int32_t* nbr_tgt = (int32_t*)(ws + l.nbr_tgt);
    int32_t* nbr_slot = (int32_t*)(ws + l.nbr_slot);
    float* nbr_d = (float*)(ws + l.nbr_d);
    int32_t* row_base = (int32_t*)(ws + l.row_base);
    int32_t* in_cnt = (int32_t*)(ws + l.in_cnt);
    int64_t* rowptr = (int64_t*)(ws + l.rowptr);
    int64_t* tiles = (int64_t*)(ws + l.tiles);
    const int64_t T = cdiv(N, SCAN_TILE);
    hipStream_t st = (hipStream_t)stream;

    if (hipMemsetAsync(in_cnt, 0, (size_t)N * 4, st) != hipSuccess) return check_launch("mdl_graph_build: memset");
    hipLaunchKernelGGL(graph_geom_kernel, dim3((unsigned)cdiv(G, 64)), dim3(64), 0, st, cell, pbc, G, geom);
    hipLaunchKernelGGL(graph_rows_kernel, dim3((unsigned)cdiv(N, 4)), dim3(256), 0, st, pos, node_ptr, geom, N, G, radius, k,
                       nbr_tgt, nbr_slot, nbr_d, row_base, in_cnt, out_deg);
    hipLaunchKernelGGL(graph_scan_tiles_kernel, dim3((unsigned)T), dim3(256), 0, st, in_cnt, N, rowptr, tiles);
    hipLaunchKernelGGL(graph_scan_top_kernel, dim3(1), dim3(256), 0, st, tiles, T, N, rowptr);
    hipLaunchKernelGGL(graph_scan_add_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, tiles, N, rowptr);
    hipLaunchKernelGGL(graph_place_kernel, dim3((unsigned)cdiv(N * k, 256)), dim3(256), 0, st, nbr_tgt, nbr_slot, nbr_d, row_base,
                       rowptr, N * k, k, src, tgt, dist);
    hipLaunchKernelGGL(graph_sort_kernel, dim3((unsigned)cdiv(N, 256)), dim3(256), 0, st, rowptr, row_base, N, src, tgt, dist);
    hipLaunchKernelGGL(graph_edge_ptr_kernel, dim3((unsigned)cdiv(G + 1, 256)), dim3(256), 0, st, node_ptr, rowptr, G, N, edge_ptr);
    return check_launch("mdl_graph_build");
}
