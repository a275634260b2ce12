// vacf.hip — what a trajectory says about TIME, sampled in front of an integrator launch of csrc/md.hip without a host read: the C
// ABI is include/mdl_hip_dynamics.h, a layer of its own behind the engine and beside csrc/observe.hip.  No reference counterpart.
//
//   mdl_md_onstep_velocity  the velocity at the evaluated positions.  Between two launches `vel` lacks the closing half kick of the
//                           step; the integrator applies it at the start of its next call (md_closed_velocity in csrc/md.hip).  The
//                           kernel restates that one statement on the same operands: one workgroup of 256 lanes per structure, an
//                           atom's row written by one lane.
//   mdl_vacf_accumulate     one workgroup of 256 lanes per (structure, live origin slot): the centre-of-mass velocity of the free
//                           atoms now and at the origin, then per type the sums of u . u0 and m u . u0, four types (eight sums) per
//                           struct_reduce.h::block_reduce; lane 0 adds into the structure's rows at the slot's lag.  Live slots
//                           have distinct lags, so one workgroup owns an accumulator word per launch: no atomics, the same bits on
//                           every run, alone and in any batch.
// fp64 throughout; contraction is off (the build flag of this file and the pragma in every kernel) and every fused multiply-add is
// written out, as in csrc/md.hip.
#include "struct_reduce.h"

#include "../../include/mdl_hip_dynamics.h"

namespace mdl {
namespace {

constexpr int DYN_THREADS = STRUCT_THREADS;

struct OnstepArgs {
    const double* vel;
    const float* force;
    const double* mass;
    const uint8_t* fixed;
    const int64_t* node_ptr;
    const double* dt;
    const int32_t *steps, *status;
    int64_t N;
    double* out;
};

__global__ __launch_bounds__(DYN_THREADS) void onstep_velocity_kernel(OnstepArgs a) {
#pragma clang fp contract(off)
    __shared__ double s_dt;
    __shared__ int32_t s_i[2];
    const int64_t b = blockIdx.x;
    int64_t n0 = a.node_ptr[b], n1 = a.node_ptr[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > a.N ? a.N : n0);
    n1 = n1 < n0 ? n0 : (n1 > a.N ? a.N : n1);
    if (threadIdx.x == 0) {
        s_dt = a.dt[b];
        s_i[0] = a.steps[b];
        s_i[1] = a.status ? a.status[b] : 0;
    }
    __syncthreads();
    if (s_i[1] != 0 || n1 == n0) return;                       // stopped, or empty: nothing of the structure is written (uniform)
    const double h = 0.5 * s_dt;
    const bool kick = s_i[0] > 0;
    const uint8_t* fixed = a.fixed;
    for (int64_t i = n0 + threadIdx.x; i < n1; i += DYN_THREADS) {
        double v[3] = {0.0, 0.0, 0.0};
        if (!(fixed && fixed[i])) {
            const double m = a.mass[i];
            // the statement of md_closed_velocity (csrc/md.hip): the closing half kick, except at the first step
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[k] = a.vel[i * 3 + k];
                if (kick) v[k] = __builtin_fma(h, (double)a.force[i * 3 + k] / m, v[k]);
            }
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a.out[i * 3 + k] = v[k];
    }
}

struct VacfArgs {
    const double *v, *origins;
    const int32_t* lag;
    const double* mass;
    const int32_t* types;
    const uint8_t* fixed;
    const int64_t* node_ptr;
    const int32_t* status;
    int64_t N;
    int32_t T, n_lags, remove_com;
    double* vacf_sum;
    int64_t* vacf_count;
};

constexpr int VACF_CHUNK = 4;                                  // types per reduction: two sums each

__global__ __launch_bounds__(DYN_THREADS) void vacf_kernel(VacfArgs a) {
#pragma clang fp contract(off)
    __shared__ double red_com[STRUCT_WAVES][7];
    __shared__ double red[STRUCT_WAVES][2 * VACF_CHUNK];
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
    const double* v0 = a.origins + k * a.N * 3;
    const uint8_t* fixed = a.fixed;

    // pass 1: the velocity of the centre of mass of the free atoms, now and at the origin
    double U[3] = {0.0, 0.0, 0.0}, U0[3] = {0.0, 0.0, 0.0};
    if (a.remove_com) {
        double acc[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t i = n0 + threadIdx.x; i < n1; i += DYN_THREADS) {
            if (fixed && fixed[i]) continue;
            const double mi = a.mass[i];
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                acc[c] = __builtin_fma(mi, a.v[i * 3 + c], acc[c]);
                acc[3 + c] = __builtin_fma(mi, v0[i * 3 + c], acc[3 + c]);
            }
            acc[6] += mi;
        }
        block_reduce<7, 7>(acc, red_com);
        if (acc[6] > 0.0) {
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                U[c] = acc[c] / acc[6];
                U0[c] = acc[3 + c] / acc[6];
            }
        }
    }
    // pass 2: per type, four types per reduction; acc[c]: sum u . u0, acc[4 + c]: sum m u . u0
    const int64_t plane = (int64_t)a.T * a.n_lags;
    double* out = a.vacf_sum + b * 2 * plane + lag;
    for (int t0 = 0; t0 < a.T; t0 += VACF_CHUNK) {
        double acc[2 * VACF_CHUNK] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        for (int64_t i = n0 + threadIdx.x; i < n1; i += DYN_THREADS) {
            if (fixed && fixed[i]) continue;
            const int32_t t = a.types[i] - t0;
            if (t < 0 || t >= VACF_CHUNK) continue;
            const double ux = a.v[i * 3 + 0] - U[0], uy = a.v[i * 3 + 1] - U[1], uz = a.v[i * 3 + 2] - U[2];
            const double wx = v0[i * 3 + 0] - U0[0], wy = v0[i * 3 + 1] - U0[1], wz = v0[i * 3 + 2] - U0[2];
            const double d = __builtin_fma(uz, wz, __builtin_fma(ux, wx, uy * wy));
            const double md = a.mass[i] * d;
#pragma unroll
            for (int c = 0; c < VACF_CHUNK; ++c) {
                acc[c] += t == c ? d : 0.0;
                acc[VACF_CHUNK + c] += t == c ? md : 0.0;
            }
        }
        block_reduce<2 * VACF_CHUNK, 2 * VACF_CHUNK>(acc, red);
        if (threadIdx.x == 0) {
#pragma unroll
            for (int c = 0; c < VACF_CHUNK; ++c)
                if (t0 + c < a.T) {
                    double* w = out + (int64_t)(t0 + c) * a.n_lags;
                    w[0] = w[0] + acc[c];
                    w[plane] = w[plane] + acc[VACF_CHUNK + c];
                }
        }
        __syncthreads();                                       // red is used again
    }
    if (threadIdx.x == 0) a.vacf_count[b * a.n_lags + lag] = a.vacf_count[b * a.n_lags + lag] + 1;
}

int dynamics_check(const char* fn, int64_t N, int64_t B) {
    MDL_REQUIRE(N >= 0 && B >= 0, MDL_E_ARG, "%s: bad N=%lld B=%lld", fn, (long long)N, (long long)B);
    MDL_REQUIRE(N == 0 || B < (1ll << 31), MDL_E_UNSUPP, "%s: B=%lld structures overflow the grid", fn, (long long)B);
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

extern "C" int mdl_md_onstep_velocity(const double* vel, const float* force, const double* mass, const uint8_t* fixed,
                                      const int64_t* node_ptr, const double* dt, const int32_t* steps, const int32_t* status, int64_t N,
                                      int64_t B, double* out, mdlStream_t stream) {
    using namespace mdl;
    const char* fn = "mdl_md_onstep_velocity";
    if (const int err = dynamics_check(fn, N, B)) return err;
    if (B == 0 || N == 0) return MDL_OK;
    MDL_REQUIRE(vel && force && mass && node_ptr && dt && steps && out, MDL_E_ARG, "%s: null pointer", fn);
    const OnstepArgs a = {vel, force, mass, fixed, node_ptr, dt, steps, status, N, out};
    hipLaunchKernelGGL(onstep_velocity_kernel, dim3((unsigned)B), dim3(DYN_THREADS), 0, (hipStream_t)stream, a);
    return check_launch(fn);
}

extern "C" int mdl_vacf_accumulate(const double* v, const double* origins, const int32_t* lag, const double* mass, const int32_t* types,
                                   const uint8_t* fixed, const int64_t* node_ptr, const int32_t* status, int64_t N, int64_t B, int32_t K,
                                   int32_t T, int32_t n_lags, int remove_com, double* vacf_sum, int64_t* vacf_count, mdlStream_t stream) {
    using namespace mdl;
    const char* fn = "mdl_vacf_accumulate";
    if (const int err = dynamics_check(fn, N, B)) return err;
    MDL_REQUIRE(K >= 0 && T >= 1 && n_lags >= 1, MDL_E_ARG, "%s: bad K=%d T=%d n_lags=%d", fn, K, T, n_lags);
    MDL_REQUIRE(T <= MDL_MSD_MAX_TYPES && K <= 65535, MDL_E_UNSUPP, "%s: T=%d (at most %d) or K=%d (at most 65535) unsupported", fn, T,
                MDL_MSD_MAX_TYPES, K);
    if (B == 0 || N == 0 || K == 0) return MDL_OK;
    MDL_REQUIRE(v && origins && lag && mass && types && node_ptr && vacf_sum && vacf_count, MDL_E_ARG, "%s: null pointer", fn);
    const VacfArgs a = {v, origins, lag, mass, types, fixed, node_ptr, status, N, T, n_lags, remove_com, vacf_sum, vacf_count};
    hipLaunchKernelGGL(vacf_kernel, dim3((unsigned)B, (unsigned)K), dim3(DYN_THREADS), 0, (hipStream_t)stream, a);
    return check_launch(fn);
}
