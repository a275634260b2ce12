// relax.hip — one FIRE update (Bitzek et al., PRL 97, 170201 (2006); unit masses) of a BATCH of structures in one launch.
// No reference counterpart: the reference has no force path and no optimiser of atomic positions.
//
//   mdl_fire_step   one workgroup of 256 lanes per structure, looping over the structure's atoms; all arithmetic fp64.
//                   pass 1: |f|^2, f.v, |v|^2 and max_i |f_i|^2 of the structure (forces of fixed atoms count as zero) -> the
//                           convergence latch and the branch of the velocity mixing, decided by every lane from the same
//                           four numbers;
//                   pass 2: v <- mix(v, f) + dt f, written, and |dt v|^2 summed;
//                   pass 3: pos += dt v, scaled to |dr| <= maxstep (the atoms are re-read from L2: a structure has at most a
//                           few hundred).
//                   Sums: wave64 shuffle tree, then the four waves through LDS in wave order — no atomics, the same bits on
//                   every run.  Lane 0 alone reads and writes the per-structure state, so no lane can see a half-updated one.
//                   A converged structure (latched before, or max_i |f_i| < fmax, or no force on a free atom) gets done = 1 and
//                   fmax_seen; nothing else of it is written.
#include "mdl_common.h"

namespace mdl {
namespace {

constexpr int FIRE_THREADS = 256;
constexpr int FIRE_WAVES = FIRE_THREADS / WAVE;

// v[0 .. NSUM) summed and v[NSUM .. K) maximised over the workgroup; every lane returns with the same totals in v.
// `red` is used once per call site (no barrier behind the read).
template <int K, int NSUM>
__device__ __forceinline__ void block_reduce(double* v, double (*red)[K]) {
#pragma unroll
    for (int k = 0; k < K; ++k)
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) {
            const double o = __shfl_down(v[k], off, WAVE);
            v[k] = k < NSUM ? v[k] + o : (o > v[k] ? o : v[k]);
        }
    const int lane = threadIdx.x % WAVE, wave = threadIdx.x / WAVE;
    if (lane == 0)
#pragma unroll
        for (int k = 0; k < K; ++k) red[wave][k] = v[k];
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) {
        double t = red[0][k];
#pragma unroll
        for (int w = 1; w < FIRE_WAVES; ++w) t = k < NSUM ? t + red[w][k] : (red[w][k] > t ? red[w][k] : t);
        v[k] = t;
    }
}

struct FireConst {
    int32_t n_min;
    double f_inc, f_dec, alpha_start, f_alpha, dt_max, maxstep;
};

__global__ __launch_bounds__(FIRE_THREADS) void fire_step_kernel(double* __restrict__ pos, double* __restrict__ vel,
                                                                 const float* __restrict__ force, const uint8_t* __restrict__ fixed,
                                                                 const int64_t* __restrict__ node_ptr, int64_t N,
                                                                 const double* __restrict__ fmax, double* dt_io, double* alpha_io,
                                                                 int32_t* n_pos_io, int32_t* steps_io, int32_t* done_io,
                                                                 float* __restrict__ fmax_seen, FireConst c) {
    __shared__ double red1[FIRE_WAVES][4];
    __shared__ double red2[FIRE_WAVES][1];
    __shared__ double st_d[3];
    __shared__ int32_t st_i[3];
    const int64_t b = blockIdx.x;
    int64_t n0 = node_ptr[b], n1 = node_ptr[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > N ? N : n0);
    n1 = n1 < n0 ? n0 : (n1 > N ? N : n1);
    if (threadIdx.x == 0) {
        st_d[0] = dt_io[b];
        st_d[1] = alpha_io[b];
        st_d[2] = fmax[b];
        st_i[0] = n_pos_io[b];
        st_i[1] = steps_io[b];
        st_i[2] = done_io[b];
    }

    // pass 1: acc = (|f|^2, f.v, |v|^2 | max_i |f_i|^2); a fixed atom has f = 0 and v = 0
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = n0 + threadIdx.x; i < n1; i += FIRE_THREADS) {
        if (fixed && fixed[i]) continue;
        const double fx = (double)force[i * 3 + 0], fy = (double)force[i * 3 + 1], fz = (double)force[i * 3 + 2];
        const double vx = vel[i * 3 + 0], vy = vel[i * 3 + 1], vz = vel[i * 3 + 2];
        const double f2 = fx * fx + fy * fy + fz * fz;
        acc[0] += f2;
        acc[1] += fx * vx + fy * vy + fz * vz;
        acc[2] += vx * vx + vy * vy + vz * vz;
        acc[3] = f2 > acc[3] ? f2 : acc[3];
    }
    block_reduce<4, 3>(acc, red1);                             // (its barrier also publishes st_d / st_i)
    const double ff = acc[0], P = acc[1], vv = acc[2], fm = sqrt(acc[3]);
    double dt = st_d[0], alpha = st_d[1];
    int32_t n_pos = st_i[0];
    const int32_t steps = st_i[1];
    const bool converged = st_i[2] != 0 || fm < st_d[2] || !(fm > 0.0);
    if (threadIdx.x == 0) fmax_seen[b] = (float)fm;
    if (converged) {                                           // uniform over the workgroup
        if (threadIdx.x == 0) done_io[b] = 1;
        return;
    }

    // velocity mixing: v <- c_v v + c_f f
    double c_v = 1.0, c_f = 0.0;
    if (steps != 0) {
        if (P > 0.0) {
            c_v = 1.0 - alpha;
            c_f = alpha * (sqrt(vv) / sqrt(ff));
            if (n_pos > c.n_min) {
                const double grown = dt * c.f_inc;
                dt = grown < c.dt_max ? grown : c.dt_max;
                alpha = alpha * c.f_alpha;
            }
            n_pos += 1;
        } else {
            c_v = 0.0;
            alpha = c.alpha_start;
            dt = dt * c.f_dec;
            n_pos = 0;
        }
    }

    // pass 2: v <- (c_v v + c_f f) + dt f;  |dt v|^2
    double s2[1] = {0.0};
    for (int64_t i = n0 + threadIdx.x; i < n1; i += FIRE_THREADS) {
        double vx = 0.0, vy = 0.0, vz = 0.0;
        if (!(fixed && fixed[i])) {
            const double fx = (double)force[i * 3 + 0], fy = (double)force[i * 3 + 1], fz = (double)force[i * 3 + 2];
            vx = (c_v * vel[i * 3 + 0] + c_f * fx) + dt * fx;
            vy = (c_v * vel[i * 3 + 1] + c_f * fy) + dt * fy;
            vz = (c_v * vel[i * 3 + 2] + c_f * fz) + dt * fz;
        }
        vel[i * 3 + 0] = vx;
        vel[i * 3 + 1] = vy;
        vel[i * 3 + 2] = vz;
        const double dx = dt * vx, dy = dt * vy, dz = dt * vz;
        s2[0] += dx * dx + dy * dy + dz * dz;
    }
    block_reduce<1, 1>(s2, red2);
    const double s = sqrt(s2[0]);
    const double clip = s > c.maxstep ? c.maxstep / s : 1.0;

    // pass 3: pos += dt v (clipped); every lane re-reads the velocities it wrote itself
    for (int64_t i = n0 + threadIdx.x; i < n1; i += FIRE_THREADS) {
        if (fixed && fixed[i]) continue;
        pos[i * 3 + 0] += (dt * vel[i * 3 + 0]) * clip;
        pos[i * 3 + 1] += (dt * vel[i * 3 + 1]) * clip;
        pos[i * 3 + 2] += (dt * vel[i * 3 + 2]) * clip;
    }
    if (threadIdx.x == 0) {
        dt_io[b] = dt;
        alpha_io[b] = alpha;
        n_pos_io[b] = n_pos;
        steps_io[b] = steps + 1;
    }
}

}  // namespace
}  // namespace mdl

extern "C" int mdl_fire_step(double* pos, double* vel, const float* force, const uint8_t* fixed, const int64_t* node_ptr, int64_t N,
                             int64_t B, const double* fmax, double* dt, double* alpha, int32_t* n_pos, int32_t* steps, int32_t* done,
                             float* fmax_seen, int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha,
                             double dt_max, double maxstep, mdlStream_t stream) {
    using namespace mdl;
    MDL_REQUIRE(N >= 0 && B >= 0, MDL_E_ARG, "mdl_fire_step: bad N=%lld B=%lld", (long long)N, (long long)B);
    MDL_REQUIRE(n_min >= 0 && f_inc > 0.0 && f_dec > 0.0 && f_alpha > 0.0 && alpha_start >= 0.0 && alpha_start <= 1.0 && dt_max > 0.0 &&
                    maxstep > 0.0,
                MDL_E_ARG, "mdl_fire_step: need n_min >= 0, f_inc, f_dec, f_alpha, dt_max, maxstep > 0 and alpha_start in [0, 1] "
                           "(got n_min=%d f_inc=%g f_dec=%g f_alpha=%g alpha_start=%g dt_max=%g maxstep=%g)",
                (int)n_min, f_inc, f_dec, f_alpha, alpha_start, dt_max, maxstep);
    if (B == 0 || N == 0) return MDL_OK;
    MDL_REQUIRE(B < (1ll << 31), MDL_E_UNSUPP, "mdl_fire_step: B=%lld structures overflow the grid", (long long)B);
    MDL_REQUIRE(pos && vel && force && node_ptr && fmax && dt && alpha && n_pos && steps && done && fmax_seen, MDL_E_ARG,
                "mdl_fire_step: null pointer");
    const FireConst c = {n_min, f_inc, f_dec, alpha_start, f_alpha, dt_max, maxstep};
    hipLaunchKernelGGL(fire_step_kernel, dim3((unsigned)B), dim3(FIRE_THREADS), 0, (hipStream_t)stream, pos, vel, force, fixed, node_ptr, N,
                       fmax, dt, alpha, n_pos, steps, done, fmax_seen, c);
    return check_launch("mdl_fire_step");
}
