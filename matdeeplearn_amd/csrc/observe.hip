// observe.hip — trajectory observables of a BATCH of structures, sampled between two steps of csrc/md.hip without a host read:
// the C ABI is include/mdl_hip_analysis.h, a layer of its own behind the engine.  No reference counterpart.
//
//   mdl_rdf_accumulate  a partial pair histogram per structure over every periodic image within r_max.  Grid (structure, tile of
//                       256 atoms i); the atoms j pass through LDS in tiles of 256.  The work items of a pass are (i, j, n_0): a
//                       lane reduces the pair's displacement to fractional coordinates in [-1/2, 1/2] once and walks the images
//                       (n_1, n_2) of its n_0, so a cell of one atom with many images and a cluster of hundreds of atoms both
//                       fill the workgroup.  Counts: 32-bit integer LDS atomics on the workgroup's histogram, flushed behind
//                       every pass to the 64-bit histogram with integer global atomics (MDL_RDF_MAX_IMAGES bounds what one pass
//                       can add to a counter below 2^32).  Integer sums: order does not matter, the bits repeat.
//   mdl_msd_accumulate  one workgroup of 256 lanes per (structure, live origin slot): the mass-weighted displacement of the free
//                       atoms' centre of mass since the origin, then per type the sum of |x - x0 - D|^2, through
//                       struct_reduce.h::block_reduce; lane 0 adds into the structure's row at the slot's lag.  Live slots have
//                       distinct lags, so one workgroup owns an accumulator word per launch: no atomics, the same bits on every
//                       run, alone and in any batch.
// fp64 throughout; contraction is off in the kernels and every fused multiply-add is written out, as in csrc/md.hip.
#include "struct_reduce.h"

#include "../../include/mdl_hip_analysis.h"

namespace mdl {
namespace {

constexpr int OBS_THREADS = STRUCT_THREADS;
constexpr int RDF_TILE = 256;                                  // atoms i per workgroup, atoms j per pass

struct RdfArgs {
    const double* pos;
    const int32_t* types;
    const int64_t* node_ptr;
    const double* cell;
    const int32_t *pbc, *status;
    int64_t N, max_atoms;
    double r_max;
    int32_t nbins, T;
    int64_t *hist, *frames;
    double* vol_sum;
    int32_t* flag;
};

__device__ __forceinline__ void cross3(const double* a, const double* b, double* c) {
#pragma clang fp contract(off)
    c[0] = a[1] * b[2] - a[2] * b[1];
    c[1] = a[2] * b[0] - a[0] * b[2];
    c[2] = a[0] * b[1] - a[1] * b[0];
}

// a <- a / |a|; false where a has no length (or is not finite)
__device__ __forceinline__ bool unit3(double* a) {
#pragma clang fp contract(off)
    const double len = sqrt(__builtin_fma(a[2], a[2], __builtin_fma(a[0], a[0], a[1] * a[1])));
    if (!(len > 0.0) || !(len < __builtin_inf())) return false;
#pragma unroll
    for (int k = 0; k < 3; ++k) a[k] = a[k] / len;
    return true;
}

// The lattice of a structure (include/mdl_hip_analysis.h, item 1), by every lane from the same numbers: A (rows; non-periodic axes
// completed by unit rows orthogonal to the periodic ones), inv = A^-1, the image range m[k] and |det| of the cell as given.
// Returns the flag bits.
__device__ __forceinline__ int rdf_lattice(const double* cell, int pbc, double r_max, double* A, double* inv, int* m, double* vol) {
#pragma clang fp contract(off)
    const bool per[3] = {(pbc & 1) != 0, (pbc & 2) != 0, (pbc & 4) != 0};
    const int np = (int)per[0] + (int)per[1] + (int)per[2];
    double R[3][3], adj[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) R[k / 3][k % 3] = cell[k];
    m[0] = m[1] = m[2] = 0;
    *vol = 0.0;
    if (np == 0) {
#pragma unroll
        for (int k = 0; k < 9; ++k) A[k] = inv[k] = (k % 4 == 0) ? 1.0 : 0.0;
        return 0;
    }
    *vol = fabs(adjugate3(cell, adj));
    bool ok = true;
    if (np == 2) {
#pragma unroll
        for (int q = 0; q < 3; ++q)
            if (!per[q]) {
                cross3(R[(q + 1) % 3], R[(q + 2) % 3], R[q]);
                ok = unit3(R[q]);
            }
    } else if (np == 1) {
#pragma unroll
        for (int p = 0; p < 3; ++p)
            if (per[p]) {
                // the coordinate axis along which the row is shortest is never parallel to it
                const double ax = fabs(R[p][0]), ay = fabs(R[p][1]), az = fabs(R[p][2]);
                const bool ex = ax <= ay && ax <= az, ey = !ex && ay <= az;
                const double e[3] = {ex ? 1.0 : 0.0, ey ? 1.0 : 0.0, (!ex && !ey) ? 1.0 : 0.0};
                cross3(R[p], e, R[(p + 1) % 3]);
                ok = unit3(R[(p + 1) % 3]);
                cross3(R[p], R[(p + 1) % 3], R[(p + 2) % 3]);
                ok = unit3(R[(p + 2) % 3]) && ok;
            }
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) A[k] = R[k / 3][k % 3];
    const double det = adjugate3(A, adj);
    if (!ok || !(fabs(det) > 0.0) || !(fabs(det) < __builtin_inf())) return MDL_RDF_NO_VOLUME;
#pragma unroll
    for (int k = 0; k < 9; ++k) inv[k] = adj[k] / det;
    int flag = 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        if (!per[k]) continue;
        // 1 / h_k = |column k of the inverse|
        const double rec = sqrt(__builtin_fma(inv[6 + k], inv[6 + k], __builtin_fma(inv[k], inv[k], inv[3 + k] * inv[3 + k])));
        const double mk = ceil(r_max * rec);
        if (!(mk <= (double)MDL_RDF_MAX_IMAGES)) flag |= rec < __builtin_inf() ? MDL_RDF_TOO_MANY_IMAGES : MDL_RDF_NO_VOLUME;
        else m[k] = (int)mk;
    }
    return flag;
}

__global__ __launch_bounds__(OBS_THREADS) void rdf_kernel(RdfArgs a) {
#pragma clang fp contract(off)
    extern __shared__ uint32_t s_hist[];                       // [P * nbins]
    __shared__ double s_xi[RDF_TILE][3], s_xj[RDF_TILE][3];
    __shared__ int32_t s_ti[RDF_TILE], s_tj[RDF_TILE];
    __shared__ double s_cell[9];
    __shared__ int32_t s_i[2], s_bad;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    int64_t n0 = a.node_ptr[b], n1 = a.node_ptr[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > a.N ? a.N : n0);
    n1 = n1 < n0 ? n0 : (n1 > a.N ? a.N : n1);
    const int64_t i0 = n0 + (int64_t)blockIdx.y * RDF_TILE;
    if (i0 >= n1) return;                                      // no such tile (an empty structure has none): uniform
    const bool first = blockIdx.y == 0;                        // the workgroup that writes what is per structure
    if (tid == 0) {
        s_i[0] = a.status ? a.status[b] : 0;
        s_i[1] = a.pbc[b] & 7;
        s_bad = 0;
        for (int k = 0; k < 9; ++k) s_cell[k] = a.cell[b * 9 + k];
    }
    __syncthreads();
    if (s_i[0] != 0) return;                                   // stopped by the integrator: nothing of the structure is written
    double C[9], A[9], inv[9], vol;
    int m[3];
#pragma unroll
    for (int k = 0; k < 9; ++k) C[k] = s_cell[k];
    const int pbc = s_i[1];
    int flag = rdf_lattice(C, pbc, a.r_max, A, inv, m, &vol);
    if (n1 - n0 > a.max_atoms) flag |= MDL_RDF_TOO_LARGE;
    if (flag != 0) {                                           // not counted (uniform)
        if (first && tid == 0) a.flag[b] = a.flag[b] | flag;
        return;
    }
    const int T = a.T, nbins = a.nbins, P = T * (T + 1) / 2, ncount = P * nbins;
    const int ni = (int)(n1 - i0 < RDF_TILE ? n1 - i0 : RDF_TILE);
    for (int c = tid; c < ncount; c += OBS_THREADS) s_hist[c] = 0u;
    if (tid < ni) {
        const int32_t t = a.types[i0 + tid];
        s_ti[tid] = (t >= 0 && t < T) ? t : -1;
#pragma unroll
        for (int k = 0; k < 3; ++k) s_xi[tid][k] = a.pos[(i0 + tid) * 3 + k];
    }
    const double scale = (double)nbins / a.r_max, r_max = a.r_max;
    const double r2_near = (r_max * r_max) * 1.000000001;      // a cheap filter in front of the square root; r < r_max decides
    const int w0 = 2 * m[0] + 1;
    int64_t* hist = a.hist + b * (int64_t)ncount;

    for (int64_t j0 = n0; j0 < n1; j0 += RDF_TILE) {
        const int nj = (int)(n1 - j0 < RDF_TILE ? n1 - j0 : RDF_TILE);
        if (tid < nj) {
            const int32_t t = a.types[j0 + tid];
            const bool good = t >= 0 && t < T;
            s_tj[tid] = good ? t : -1;
            if (!good) s_bad = 1;                              // (every writer stores the same word)
#pragma unroll
            for (int k = 0; k < 3; ++k) s_xj[tid][k] = a.pos[(j0 + tid) * 3 + k];
        }
        __syncthreads();
        const int items = ni * nj * w0;                        // <= 256 * 256 * 33
        for (int q = tid; q < items; q += OBS_THREADS) {
            const int pr = q / w0, i = pr / nj, j = pr - i * nj;
            const int ti = s_ti[i], tj = s_tj[j];
            if (ti < 0 || tj < 0) continue;
            const int lo = ti < tj ? ti : tj, hi = ti < tj ? tj : ti;
            uint32_t* h = s_hist + (lo * T - lo * (lo - 1) / 2 + (hi - lo)) * nbins;
            const bool self = i0 + i == j0 + j;
            double d[3], s[3], base[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) d[k] = s_xj[j][k] - s_xi[i][k];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                const double f = __builtin_fma(d[2], inv[6 + k], __builtin_fma(d[1], inv[3 + k], d[0] * inv[k]));
                s[k] = (pbc >> k) & 1 ? rint(f) : 0.0;
            }
            const int e0 = q - pr * w0 - m[0];
            const double g0 = (double)e0 - s[0];               // the image n_0 of the reduced displacement
#pragma unroll
            for (int k = 0; k < 3; ++k) base[k] = __builtin_fma(g0, A[k], d[k]);
            for (int e1 = -m[1]; e1 <= m[1]; ++e1) {
                const double g1 = (double)e1 - s[1];
                double u[3];
#pragma unroll
                for (int k = 0; k < 3; ++k) u[k] = __builtin_fma(g1, A[3 + k], base[k]);
                for (int e2 = -m[2]; e2 <= m[2]; ++e2) {
                    if (self && e0 == 0 && e1 == 0 && e2 == 0) continue;
                    const double g2 = (double)e2 - s[2];
                    const double vx = __builtin_fma(g2, A[6], u[0]), vy = __builtin_fma(g2, A[7], u[1]), vz = __builtin_fma(g2, A[8], u[2]);
                    const double r2 = __builtin_fma(vz, vz, __builtin_fma(vx, vx, vy * vy));
                    if (!(r2 < r2_near)) continue;             // (a NaN is not counted)
                    const double r = sqrt(r2);
                    if (!(r < r_max)) continue;
                    int bin = (int)(r * scale);
                    bin = bin < nbins ? bin : nbins - 1;
                    atomicAdd(h + bin, 1u);
                }
            }
        }
        __syncthreads();
        // the flush behind every pass: no counter has seen more than 256 * 256 * 33^3 < 2^32 adds
        for (int c = tid; c < ncount; c += OBS_THREADS) {
            const uint32_t v = s_hist[c];
            if (v != 0u) {
                atomicAdd(reinterpret_cast<unsigned long long*>(hist + c), (unsigned long long)v);
                s_hist[c] = 0u;
            }
        }
        __syncthreads();
    }
    if (first && tid == 0) {                                   // one add per frame
        a.frames[b] = a.frames[b] + 1;
        a.vol_sum[b] = a.vol_sum[b] + vol;
        if (s_bad) a.flag[b] = a.flag[b] | MDL_RDF_BAD_TYPE;
    }
}

struct MsdArgs {
    const double *pos, *origins;
    const int32_t* lag;
    const double* mass;
    const int32_t* types;
    const uint8_t* fixed;
    const int64_t* node_ptr;
    const int32_t* status;
    int64_t N;
    int32_t T, n_lags, remove_com;
    double* msd_sum;
    int64_t* msd_count;
};

constexpr int MSD_CHUNK = 4;                                   // types per reduction

__global__ __launch_bounds__(OBS_THREADS) void msd_kernel(MsdArgs a) {
#pragma clang fp contract(off)
    __shared__ double red[STRUCT_WAVES][MSD_CHUNK];
    __shared__ int32_t s_i[2];
    const int64_t b = blockIdx.x, k = blockIdx.y;
    int64_t n0 = a.node_ptr[b], n1 = a.node_ptr[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > a.N ? a.N : n0);
    n1 = n1 < n0 ? n0 : (n1 > a.N ? a.N : n1);
    if (threadIdx.x == 0) {
        s_i[0] = a.lag[k];
        s_i[1] = a.status ? a.status[b] : 0;
    }
    __syncthreads();
    const int32_t lag = s_i[0];
    if (lag < 0 || lag >= a.n_lags || s_i[1] != 0 || n1 == n0) return;              // uniform
    const double* x0 = a.origins + k * a.N * 3;
    const uint8_t* fixed = a.fixed;

    // pass 1: the displacement of the centre of mass of the free atoms since the origin
    double D[3] = {0.0, 0.0, 0.0};
    if (a.remove_com) {
        double acc[MSD_CHUNK] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t i = n0 + threadIdx.x; i < n1; i += OBS_THREADS) {
            if (fixed && fixed[i]) continue;
            const double mi = a.mass[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) acc[c] = __builtin_fma(mi, a.pos[i * 3 + c] - x0[i * 3 + c], acc[c]);
            acc[3] += mi;
        }
        block_reduce<MSD_CHUNK, MSD_CHUNK>(acc, red);
        if (acc[3] > 0.0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) D[c] = acc[c] / acc[3];
        }
        __syncthreads();                                       // red is used again
    }
    // pass 2: per type, four types per reduction
    double* out = a.msd_sum + (b * a.T) * (int64_t)a.n_lags + lag;
    for (int t0 = 0; t0 < a.T; t0 += MSD_CHUNK) {
        double acc[MSD_CHUNK] = {0.0, 0.0, 0.0, 0.0};
        for (int64_t i = n0 + threadIdx.x; i < n1; i += OBS_THREADS) {
            if (fixed && fixed[i]) continue;
            const int32_t t = a.types[i] - t0;
            if (t < 0 || t >= MSD_CHUNK) continue;
            const double ux = (a.pos[i * 3 + 0] - x0[i * 3 + 0]) - D[0], uy = (a.pos[i * 3 + 1] - x0[i * 3 + 1]) - D[1];
            const double uz = (a.pos[i * 3 + 2] - x0[i * 3 + 2]) - D[2];
            const double u2 = __builtin_fma(uz, uz, __builtin_fma(ux, ux, uy * uy));
#pragma unroll
            for (int c = 0; c < MSD_CHUNK; ++c) acc[c] += t == c ? u2 : 0.0;
        }
        block_reduce<MSD_CHUNK, MSD_CHUNK>(acc, red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < MSD_CHUNK; ++c)
                if (t0 + c < a.T) out[(int64_t)(t0 + c) * a.n_lags] = out[(int64_t)(t0 + c) * a.n_lags] + acc[c];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) a.msd_count[b * a.n_lags + lag] = a.msd_count[b * a.n_lags + lag] + 1;
}

int observe_check(const char* fn, int64_t N, int64_t B) {
    MDL_REQUIRE(N >= 0 && B >= 0, MDL_E_ARG, "%s: bad N=%lld B=%lld", fn, (long long)N, (long long)B);
    MDL_REQUIRE(N == 0 || B < (1ll << 31), MDL_E_UNSUPP, "%s: B=%lld structures overflow the grid", fn, (long long)B);
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

extern "C" int mdl_rdf_accumulate(const double* pos, const int32_t* types, const int64_t* node_ptr, const double* cell, const int32_t* pbc,
                                  const int32_t* status, int64_t N, int64_t B, int64_t max_atoms, double r_max, int32_t nbins, int32_t T,
                                  int64_t* hist, int64_t* frames, double* vol_sum, int32_t* flag, mdlStream_t stream) {
    using namespace mdl;
    const char* fn = "mdl_rdf_accumulate";
    if (const int err = observe_check(fn, N, B)) return err;
    MDL_REQUIRE(r_max > 0.0 && r_max < __builtin_inf(), MDL_E_ARG, "%s: r_max must be > 0 and finite (got %g)", fn, r_max);
    MDL_REQUIRE(nbins >= 1 && T >= 1 && max_atoms >= 0, MDL_E_ARG, "%s: bad nbins=%d T=%d max_atoms=%lld", fn, nbins, T, (long long)max_atoms);
    const int64_t counters = (int64_t)T * (T + 1) / 2 * nbins;
    MDL_REQUIRE(counters <= MDL_RDF_MAX_COUNTERS, MDL_E_UNSUPP, "%s: T (T + 1) / 2 * nbins = %lld counters exceed the LDS histogram of %d", fn,
                (long long)counters, MDL_RDF_MAX_COUNTERS);
    const int64_t tiles = cdiv(max_atoms < N ? max_atoms : N, RDF_TILE);
    MDL_REQUIRE(tiles <= 65535, MDL_E_UNSUPP, "%s: max_atoms=%lld needs more than 65535 tiles", fn, (long long)max_atoms);
    if (B == 0 || N == 0 || tiles == 0) return MDL_OK;
    MDL_REQUIRE(pos && types && node_ptr && cell && pbc && hist && frames && vol_sum && flag, MDL_E_ARG, "%s: null pointer", fn);
    const RdfArgs a = {pos, types, node_ptr, cell, pbc, status, N, max_atoms, r_max, nbins, T, hist, frames, vol_sum, flag};
    hipLaunchKernelGGL(rdf_kernel, dim3((unsigned)B, (unsigned)tiles), dim3(OBS_THREADS), (size_t)counters * sizeof(uint32_t),
                       (hipStream_t)stream, a);
    return check_launch(fn);
}

extern "C" int mdl_msd_accumulate(const double* pos, const double* origins, const int32_t* lag, const double* mass, const int32_t* types,
                                  const uint8_t* fixed, const int64_t* node_ptr, const int32_t* status, int64_t N, int64_t B, int32_t K,
                                  int32_t T, int32_t n_lags, int remove_com, double* msd_sum, int64_t* msd_count, mdlStream_t stream) {
    using namespace mdl;
    const char* fn = "mdl_msd_accumulate";
    if (const int err = observe_check(fn, N, B)) return err;
    MDL_REQUIRE(K >= 0 && T >= 1 && n_lags >= 1, MDL_E_ARG, "%s: bad K=%d T=%d n_lags=%d", fn, K, T, n_lags);
    MDL_REQUIRE(T <= MDL_MSD_MAX_TYPES && K <= 65535, MDL_E_UNSUPP, "%s: T=%d (at most %d) or K=%d (at most 65535) unsupported", fn, T,
                MDL_MSD_MAX_TYPES, K);
    if (B == 0 || N == 0 || K == 0) return MDL_OK;
    MDL_REQUIRE(pos && origins && lag && mass && types && node_ptr && msd_sum && msd_count, MDL_E_ARG, "%s: null pointer", fn);
    const MsdArgs a = {pos, origins, lag, mass, types, fixed, node_ptr, status, N, T, n_lags, remove_com, msd_sum, msd_count};
    hipLaunchKernelGGL(msd_kernel, dim3((unsigned)B, (unsigned)K), dim3(OBS_THREADS), 0, (hipStream_t)stream, a);
    return check_launch(fn);
}
