// sq.hip — what a trajectory says in RECIPROCAL space, sampled between two integrator launches without a host read: the C ABI is
// include/mdl_hip_scattering.h, a layer of its own behind the engine and beside csrc/observe.hip and csrc/vacf.hip.  No reference
// counterpart.
//
//   mdl_density_modes   rho_t(q) = sum over the atoms of type t of exp(-i q . x) at Q reciprocal-lattice vectors q = 2 pi n C^-T.
//                       Grid (structure, tile of 256 q), one q per lane.  The atoms pass through LDS in chunks of 256: the loading
//                       lane forms its atom's fractional coordinates once, every lane then walks the chunk with broadcast reads
//                       (one address per wave: no bank conflict) and adds into ITS column of the [T][256] complex accumulators,
//                       which live in LDS because a register array indexed by the atom's type would go to scratch.  No cross-lane
//                       reduction and no atomics: the sum of a (type, q) is a sequential one in ascending atom index.
//   mdl_sq_accumulate   the symmetrised real part of rho_a conj(rho0_c) per pair of types and q, against every live slot of a ring
//                       of stored modes (into f_sum at the slot's lag) and against the frame itself (into s_sum).  Grid (structure,
//                       slot, tile of 256 q); a lane walks the pairs.  Live slots have distinct lags, so one lane owns an
//                       accumulator word per launch.
// fp64 throughout; contraction is off (the build flag of this file and the pragma in every kernel), as in csrc/vacf.hip.
#include "struct_reduce.h"

#include "../../include/mdl_hip_scattering.h"

namespace mdl {
namespace {

constexpr int SQ_THREADS = 256;                                // one q per lane: the q-tile, and the chunk of atoms in LDS

struct ModesArgs {
    const double* pos;
    const int32_t* types;
    const int64_t* node_ptr;
    const double* cell;
    const int32_t *pbc, *status, *qvec;
    int64_t N;
    int32_t Q, T;
    double* rho;
    int64_t* frames;
    double* cell_sum;
    int32_t* flag;
};

__global__ __launch_bounds__(SQ_THREADS) void density_modes_kernel(ModesArgs a) {
#pragma clang fp contract(off)
    extern __shared__ double2 s_acc[];                         // [T][SQ_THREADS] (re, im)
    __shared__ double s_f[3][SQ_THREADS];
    __shared__ int32_t s_t[SQ_THREADS];
    __shared__ double s_cell[9];
    __shared__ int32_t s_i[3], s_bad;
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x;
    int64_t n0 = a.node_ptr[b], n1 = a.node_ptr[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > a.N ? a.N : n0);
    n1 = n1 < n0 ? n0 : (n1 > a.N ? a.N : n1);
    if (n1 == n0) return;                                      // empty: nothing of the structure is written (uniform)
    const bool first = blockIdx.y == 0;                        // the workgroup that writes what is per structure
    if (tid == 0) {
        s_i[0] = a.status ? a.status[b] : 0;
        s_i[1] = a.pbc[b] & 7;
        // only the fatal bits are looked at: they are written by no workgroup of this launch unless every workgroup of the structure
        // derives them itself from pbc and the cell below
        s_i[2] = a.flag[b] & MDL_SQ_FATAL;
        s_bad = 0;
        for (int k = 0; k < 9; ++k) s_cell[k] = a.cell[b * 9 + k];
    }
    __syncthreads();
    if (s_i[0] != 0 || s_i[2] != 0) return;                    // stopped by the integrator, or flagged earlier (uniform)
    double C[9], adj[9], inv[9];
#pragma unroll
    for (int k = 0; k < 9; ++k) C[k] = s_cell[k];
    int bits = s_i[1] != 7 ? MDL_SQ_NOT_PERIODIC : 0;
    const double det = adjugate3(C, adj);
    bool finite = true;
#pragma unroll
    for (int k = 0; k < 9; ++k) finite = finite && fabs(C[k]) < __builtin_inf();
    if (!finite || !(fabs(det) > 0.0) || !(fabs(det) < __builtin_inf())) bits |= MDL_SQ_NO_VOLUME;
    if (bits != 0) {                                           // not counted (uniform)
        if (first && tid == 0) a.flag[b] = a.flag[b] | bits;
        return;
    }
#pragma unroll
    for (int k = 0; k < 9; ++k) inv[k] = adj[k] / det;
    const int T = a.T;
    const int64_t q = (int64_t)blockIdx.y * SQ_THREADS + tid;
    const bool live = q < a.Q;
    double n[3] = {0.0, 0.0, 0.0};
    if (live) {
#pragma unroll
        for (int k = 0; k < 3; ++k) n[k] = (double)a.qvec[q * 3 + k];
    }
    for (int t = 0; t < T; ++t) s_acc[t * SQ_THREADS + tid] = make_double2(0.0, 0.0);      // a lane's own column: no barrier needed
    for (int64_t c0 = n0; c0 < n1; c0 += SQ_THREADS) {
        const int cnt = (int)(n1 - c0 < SQ_THREADS ? n1 - c0 : SQ_THREADS);
        __syncthreads();                                       // the chunk before this one has been walked by every lane
        if (tid < cnt) {
            const int64_t i = c0 + tid;
            const double x0 = a.pos[i * 3 + 0], x1 = a.pos[i * 3 + 1], x2 = a.pos[i * 3 + 2];
#pragma unroll
            for (int k = 0; k < 3; ++k) s_f[k][tid] = (x0 * inv[k] + x1 * inv[3 + k]) + x2 * inv[6 + k];
            const int32_t t = a.types[i];
            const bool ok = t >= 0 && t < T;
            s_t[tid] = ok ? t : -1;
            if (!ok) s_bad = 1;                                // (every writer writes the same value)
        }
        __syncthreads();
        if (live) {
            for (int j = 0; j < cnt; ++j) {
                const int32_t t = s_t[j];                      // one address per wave: a broadcast, and a uniform branch
                if (t < 0) continue;
                const double phi = (n[0] * s_f[0][j] + n[1] * s_f[1][j]) + n[2] * s_f[2][j];
                const double r = phi - rint(phi);
                double s, c;
                sincospi(2.0 * r, &s, &c);
                double2 acc = s_acc[t * SQ_THREADS + tid];
                acc.x = acc.x + c;
                acc.y = acc.y - s;
                s_acc[t * SQ_THREADS + tid] = acc;
            }
        }
    }
    if (live) {
        double2* out = reinterpret_cast<double2*>(a.rho) + (b * T) * (int64_t)a.Q + q;
        for (int t = 0; t < T; ++t) out[(int64_t)t * a.Q] = s_acc[t * SQ_THREADS + tid];
    }
    if (first && tid == 0) {                                   // (s_bad: the barrier behind the last chunk's loads has passed)
        a.frames[b] = a.frames[b] + 1;
#pragma unroll
        for (int k = 0; k < 9; ++k) a.cell_sum[b * 9 + k] = a.cell_sum[b * 9 + k] + C[k];
        if (s_bad) a.flag[b] = a.flag[b] | MDL_SQ_BAD_TYPE;
    }
}

struct SqArgs {
    const double *rho, *origins;
    const int32_t *lag, *flag, *status;
    const int64_t* node_ptr;
    int64_t N, B;
    int32_t K, T, Q, n_lags;
    double *s_sum, *f_sum;
    int64_t* f_count;
};

// one q of one structure: for every pair (a <= c) dst[pair * stride] += 0.5 * ((R_a.re O_c.re + R_a.im O_c.im) + (R_c.re O_a.re + R_c.im O_a.im));
// R, O and dst point at the lane's q of type 0 / pair 0
__device__ __forceinline__ void sq_pairs(const double2* R, const double2* O, double* dst, int T, int64_t Q, int64_t stride) {
#pragma clang fp contract(off)
    int pair = 0;
    for (int ta = 0; ta < T; ++ta) {
        const double2 ra = R[ta * Q], oa = O[ta * Q];
        for (int tc = ta; tc < T; ++tc, ++pair) {
            const double2 rc = R[tc * Q], oc = O[tc * Q];
            const double w = 0.5 * ((ra.x * oc.x + ra.y * oc.y) + (rc.x * oa.x + rc.y * oa.y));
            dst[pair * stride] = dst[pair * stride] + w;
        }
    }
}

__global__ __launch_bounds__(SQ_THREADS) void sq_accumulate_kernel(SqArgs a) {
#pragma clang fp contract(off)
    __shared__ int32_t s_i[3];
    const int tid = threadIdx.x;
    const int64_t b = blockIdx.x, k = blockIdx.y;
    int64_t n0 = a.node_ptr[b], n1 = a.node_ptr[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > a.N ? a.N : n0);
    n1 = n1 < n0 ? n0 : (n1 > a.N ? a.N : n1);
    if (tid == 0) {
        s_i[0] = a.K > 0 ? a.lag[k] : -1;
        s_i[1] = a.status ? a.status[b] : 0;
        s_i[2] = a.flag[b] & MDL_SQ_FATAL;
    }
    __syncthreads();
    if (s_i[1] != 0 || s_i[2] != 0 || n1 == n0) return;        // uniform
    const int T = a.T, P = T * (T + 1) / 2;
    const int64_t Q = a.Q, q = (int64_t)blockIdx.z * SQ_THREADS + tid;
    const int32_t lag = s_i[0];
    const bool slot = lag >= 0 && lag < a.n_lags;
    const double2* R = reinterpret_cast<const double2*>(a.rho) + b * T * Q + q;
    if (q < Q) {
        if (slot) {
            const double2* O = reinterpret_cast<const double2*>(a.origins) + (k * a.B + b) * T * Q + q;
            sq_pairs(R, O, a.f_sum + (b * P * a.n_lags + lag) * Q + q, T, Q, (int64_t)a.n_lags * Q);
        }
        if (k == 0) sq_pairs(R, R, a.s_sum + b * P * Q + q, T, Q, Q);      // the self slot rides with the first slot's workgroups
    }
    if (slot && blockIdx.z == 0 && tid == 0) a.f_count[b * a.n_lags + lag] = a.f_count[b * a.n_lags + lag] + 1;
}

int scattering_check(const char* fn, int64_t N, int64_t B, int32_t Q, int32_t T) {
    MDL_REQUIRE(N >= 0 && B >= 0 && Q >= 0, MDL_E_ARG, "%s: bad N=%lld B=%lld Q=%d", fn, (long long)N, (long long)B, Q);
    MDL_REQUIRE(T >= 1, MDL_E_ARG, "%s: bad T=%d", fn, T);
    MDL_REQUIRE(T <= MDL_SQ_MAX_TYPES, MDL_E_UNSUPP, "%s: T=%d types (at most %d) unsupported", fn, T, MDL_SQ_MAX_TYPES);
    MDL_REQUIRE(B < (1ll << 31), MDL_E_UNSUPP, "%s: B=%lld structures overflow the grid", fn, (long long)B);
    MDL_REQUIRE(((int64_t)Q + SQ_THREADS - 1) / SQ_THREADS <= 65535, MDL_E_UNSUPP, "%s: Q=%d needs more than 65535 q-tiles", fn, Q);
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

extern "C" int mdl_density_modes(const double* pos, const int32_t* types, const int64_t* node_ptr, const double* cell, const int32_t* pbc,
                                 const int32_t* status, const int32_t* qvec, int64_t N, int64_t B, int32_t Q, int32_t T, double* rho,
                                 int64_t* frames, double* cell_sum, int32_t* flag, mdlStream_t stream) {
    using namespace mdl;
    const char* fn = "mdl_density_modes";
    if (const int err = scattering_check(fn, N, B, Q, T)) return err;
    if (B == 0 || N == 0 || Q == 0) return MDL_OK;
    MDL_REQUIRE(pos && types && node_ptr && cell && pbc && qvec && rho && frames && cell_sum && flag, MDL_E_ARG, "%s: null pointer", fn);
    const ModesArgs a = {pos, types, node_ptr, cell, pbc, status, qvec, N, Q, T, rho, frames, cell_sum, flag};
    const unsigned tiles = (unsigned)((Q + SQ_THREADS - 1) / SQ_THREADS);
    hipLaunchKernelGGL(density_modes_kernel, dim3((unsigned)B, tiles), dim3(SQ_THREADS), (size_t)T * SQ_THREADS * sizeof(double2),
                       (hipStream_t)stream, a);
    return check_launch(fn);
}

extern "C" int mdl_sq_accumulate(const double* rho, const double* origins, const int32_t* lag, const int32_t* flag, const int32_t* status,
                                 const int64_t* node_ptr, int64_t N, int64_t B, int32_t K, int32_t T, int32_t Q, int32_t n_lags,
                                 double* s_sum, double* f_sum, int64_t* f_count, mdlStream_t stream) {
    using namespace mdl;
    const char* fn = "mdl_sq_accumulate";
    if (const int err = scattering_check(fn, N, B, Q, T)) return err;
    MDL_REQUIRE(K >= 0 && n_lags >= 1, MDL_E_ARG, "%s: bad K=%d n_lags=%d", fn, K, n_lags);
    MDL_REQUIRE(K <= 65535, MDL_E_UNSUPP, "%s: K=%d slots (at most 65535) unsupported", fn, K);
    if (B == 0 || N == 0 || Q == 0) return MDL_OK;
    MDL_REQUIRE(rho && flag && node_ptr && s_sum && (K == 0 || (origins && lag && f_sum && f_count)), MDL_E_ARG, "%s: null pointer", fn);
    const SqArgs a = {rho, origins, lag, flag, status, node_ptr, N, B, K, T, Q, n_lags, s_sum, f_sum, f_count};
    const unsigned tiles = (unsigned)((Q + SQ_THREADS - 1) / SQ_THREADS);
    hipLaunchKernelGGL(sq_accumulate_kernel, dim3((unsigned)B, (unsigned)(K > 0 ? K : 1), tiles), dim3(SQ_THREADS), 0, (hipStream_t)stream, a);
    return check_launch(fn);
}
