// md.hip — molecular dynamics of a BATCH of structures: everything between two force evaluations in one launch.
// No reference counterpart: the reference has no force path and moves no atoms.
//
//   mdl_md_step        BAOAB (Leimkuhler & Matthews, J. Chem. Phys. 138, 174102 (2013)) with ONE force evaluation per step: the
//                      closing half kick of step n and B A O A of step n + 1 are one call.  One workgroup of 256 lanes per
//                      structure, looping over the structure's atoms; all arithmetic fp64.
//                      pass 1: v <- v + h f / m (the closing kick, not at steps == 0), the kinetic energy of that v, and — from
//                              the candidate x'', v'' of the same atom — the number of free atoms that would move further than
//                              max_disp (a NaN counts); nothing is written;
//                      pass 2: the branch all lanes take from those two sums: the closing call (steps == n_steps) and a refused
//                              step store the v of pass 1, an accepted step the candidate, formed again by the same statements.
//                      An atom's row is read and written by one lane only, so the update is in place.
//                      The cell mode (cell != NULL) adds an isotropic barostat, stochastic cell rescaling (Bernetti & Bussi,
//                      J. Chem. Phys. 153, 114107 (2020)) in eps = ln V: behind the sum for the kinetic energy every lane forms
//                      volume, pressure and the strain d eps of the step from the same numbers; positions and cell are scaled by
//                      s = exp(d eps / 3), velocities by 1 / s, and B A O A starts from the scaled pair.  The forces are those of
//                      the UNSCALED positions: first-order splitting, as in the paper's own integrator.
//   mdl_md_velocities  Maxwell-Boltzmann velocities from the same noise, the centre-of-mass velocity of the free atoms removed.
// Noise: Philox4x32-10 (Salmon et al., SC'11) keyed by the structure's seed and counted by (atom within the structure, 0, step,
// tag), so a structure's random numbers do not depend on the batch it is in, on the launch or on the process; Box-Muller on
// u = (w + 0.5) 2^-32, which is never 0 or 1.
// Sums: struct_reduce.h — wave64 shuffle tree, then the four waves through LDS in wave order; no atomics, the same bits on every
// run.  Lane 0 alone reads and writes the per-structure state.  Contraction is off in the kernels and every fused multiply-add is
// written out, as in csrc/relax.hip.
#include "struct_reduce.h"

namespace mdl {
namespace {

constexpr int MD_THREADS = STRUCT_THREADS;
constexpr uint32_t MD_TAG_THERMOSTAT = 0, MD_TAG_VELOCITIES = 1, MD_TAG_BAROSTAT = 2;

// Philox4x32-10: counter c[4], key (k0, k1) -> c
__device__ __forceinline__ void philox4x32_10(uint32_t* c, uint32_t k0, uint32_t k1) {
    constexpr uint32_t M0 = 0xD2511F53u, M1 = 0xCD9E8D57u, W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint32_t hi0 = __umulhi(M0, c[0]), lo0 = M0 * c[0];
        const uint32_t hi1 = __umulhi(M1, c[2]), lo1 = M1 * c[2];
        c[0] = hi1 ^ c[1] ^ k0;
        c[1] = lo1;
        c[2] = hi0 ^ c[3] ^ k1;
        c[3] = lo0;
        k0 += W0;
        k1 += W1;
    }
}

// three standard normal numbers of atom `atom` (its index within the structure) at step word `step`
__device__ __forceinline__ void md_noise(uint32_t atom, uint32_t step, uint32_t tag, int64_t seed, double* xi) {
#pragma clang fp contract(off)
    uint32_t w[4] = {atom, 0u, step, tag};
    philox4x32_10(w, (uint32_t)((uint64_t)seed & 0xffffffffull), (uint32_t)((uint64_t)seed >> 32));
    constexpr double INV32 = 1.0 / 4294967296.0;
    const double u0 = ((double)w[0] + 0.5) * INV32, u1 = ((double)w[1] + 0.5) * INV32;
    const double u2 = ((double)w[2] + 0.5) * INV32, u3 = ((double)w[3] + 0.5) * INV32;
    const double r0 = sqrt(-2.0 * log(u0)), r1 = sqrt(-2.0 * log(u2));
    // cos and sin of 2 pi u as cospi / sinpi of 2 u (exact): no argument reduction against a rounded pi, and none that needs a stack
    xi[0] = r0 * cospi(2.0 * u1);
    xi[1] = r0 * sinpi(2.0 * u1);
    xi[2] = r1 * cospi(2.0 * u3);
}

struct MdArgs {
    double *pos, *vel;
    const float* force;
    const double* mass;
    const uint8_t* fixed;
    const int64_t* node_ptr;
    int64_t N;
    const double *dt, *gamma, *kT;
    const int64_t* seed;
    const int32_t* n_steps;
    int32_t *steps, *status;
    double* ekin;
    // the cell mode
    double* cell;
    const float* strain_grad;
    const double *pressure, *baro_rate;
    double *volume, *press;
};

// what one atom needs of its structure
struct MdStep {
    double h, c1, c2, kT;
    int64_t seed;
    uint32_t step;
    bool kick, thermostat;
};

// the v of item 2 (include/mdl_hip.h, mdl_md_step) of free atom i: the closing half kick, except at the first step
__device__ __forceinline__ void md_closed_velocity(const MdArgs& a, const MdStep& s, int64_t i, double m, double* v) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        v[k] = a.vel[i * 3 + k];
        if (s.kick) v[k] = __builtin_fma(s.h, (double)a.force[i * 3 + k] / m, v[k]);
    }
}

// B A O A of free atom i from the position x and the velocity v (the row of pos and the v of item 2; in the cell mode both scaled
// by the barostat): x'' and v''; returns |x'' - x|
__device__ __forceinline__ double md_candidate(const MdArgs& a, const MdStep& s, int64_t i, uint32_t atom, double m, const double* x,
                                               const double* v, double* xn, double* vn) {
#pragma clang fp contract(off)
    double xi[3] = {0.0, 0.0, 0.0}, sigma = 0.0;
    if (s.thermostat) {
        md_noise(atom, s.step, MD_TAG_THERMOSTAT, s.seed, xi);
        sigma = s.c2 * sqrt(s.kT / m);
    }
    double d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double v1 = __builtin_fma(s.h, (double)a.force[i * 3 + k] / m, v[k]);
        const double x1 = __builtin_fma(s.h, v1, x[k]);
        vn[k] = s.thermostat ? __builtin_fma(sigma, xi[k], s.c1 * v1) : v1;
        xn[k] = __builtin_fma(s.h, vn[k], x1);
        d[k] = xn[k] - x[k];
    }
    return sqrt(__builtin_fma(d[2], d[2], __builtin_fma(d[0], d[0], d[1] * d[1])));
}

// what the candidate of free atom i starts from: its row of pos and the v of item 2, or — where the barostat acts — s x and v / s
__device__ __forceinline__ void md_start(const MdArgs& a, int64_t i, bool baro, double sc, const double* v, double* xs, double* vs) {
#pragma clang fp contract(off)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const double x = a.pos[i * 3 + k];
        xs[k] = baro ? sc * x : x;
        vs[k] = baro ? v[k] / sc : v[k];
    }
}

// ONE kernel body, instantiated twice.
// CELL = false: the atoms alone (include/mdl_hip.h, mdl_md_step with cell == NULL): one reduction carries both sums, and no cell
// pointer is touched.
// CELL = true: the cell mode.  The barostat needs the kinetic energy before the candidate can be formed, so the sums are two
// reductions: ekin, then — behind the barostat's decision, which every lane takes from the same numbers — n_bad on the scaled
// candidate.  A structure with rate == 0 runs the statements of CELL = false on the same operands: the same bits.
template <bool CELL>
__global__ __launch_bounds__(MD_THREADS) void md_step_kernel(MdArgs a, double max_disp, double max_strain) {
#pragma clang fp contract(off)
    __shared__ double red[STRUCT_WAVES][CELL ? 1 : 2];
    __shared__ double red2[STRUCT_WAVES][1];                   // CELL only
    __shared__ double st_d[5];
    __shared__ int64_t st_seed;
    __shared__ int32_t st_i[3];
    __shared__ double m_C[9], m_S[3];                          // CELL only: the cell and the diagonal of dE/d eps
    const int64_t b = blockIdx.x;
    int64_t n0 = a.node_ptr[b], n1 = a.node_ptr[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > a.N ? a.N : n0);
    n1 = n1 < n0 ? n0 : (n1 > a.N ? a.N : n1);
    if (threadIdx.x == 0) {
        st_d[0] = a.dt[b];
        st_d[1] = a.gamma[b];
        st_d[2] = a.kT[b];
        st_seed = a.seed[b];
        st_i[0] = a.n_steps[b];
        st_i[1] = a.steps[b];
        st_i[2] = a.status[b];
        if constexpr (CELL) {
            st_d[3] = a.pressure[b];
            st_d[4] = a.baro_rate[b];
            for (int k = 0; k < 9; ++k) m_C[k] = a.cell[b * 9 + k];
            for (int k = 0; k < 3; ++k) m_S[k] = (double)a.strain_grad[b * 9 + 4 * k];
        }
    }
    __syncthreads();
    if (st_i[2] != 0) return;                                  // stopped before: nothing of the structure is written (uniform)
    const double dt = st_d[0], gamma = st_d[1];
    const int32_t steps = st_i[1];
    const bool closing = steps == st_i[0];
    MdStep s;
    s.h = 0.5 * dt;
    s.kT = st_d[2];
    s.seed = st_seed;
    s.step = (uint32_t)steps;
    s.kick = steps > 0;
    s.thermostat = gamma > 0.0;
    s.c1 = 1.0;
    s.c2 = 0.0;
    if (s.thermostat) {                                        // every lane from the same two numbers
        s.c1 = exp(-(gamma * dt));
        s.c2 = sqrt(-expm1(-(2.0 * (gamma * dt))));
    }
    const uint8_t* fixed = a.fixed;

    // pass 1: acc = (sum m |v|^2, the number of free atoms whose candidate is not within max_disp); CELL: the first sum alone
    double acc[2] = {0.0, 0.0};
    for (int64_t i = n0 + threadIdx.x; i < n1; i += MD_THREADS) {
        if (fixed && fixed[i]) continue;
        const double m = a.mass[i];
        double v[3], xn[3], vn[3];
        md_closed_velocity(a, s, i, m, v);
        acc[0] += m * __builtin_fma(v[2], v[2], __builtin_fma(v[0], v[0], v[1] * v[1]));
        if constexpr (!CELL)
            if (!closing) acc[1] += md_candidate(a, s, i, (uint32_t)(i - n0), m, a.pos + i * 3, v, xn, vn) <= max_disp ? 0.0 : 1.0;
    }
    block_reduce<CELL ? 1 : 2, CELL ? 1 : 2>(acc, red);

    // CELL: volume and pressure, the barostat's strain and its guard — every lane from the same numbers
    bool baro = false, strained = false;
    double sc = 1.0, C[9];
    if constexpr (CELL) {
        double adj[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) C[k] = m_C[k];
        const double V = fabs(adjugate3(C, adj));
        const bool has_volume = V > 0.0;                       // (a NaN has none)
        const double P = has_volume ? (acc[0] - (m_S[0] + m_S[1] + m_S[2])) / (3.0 * V) : __builtin_nan("");
        if (threadIdx.x == 0) {
            a.volume[b] = has_volume ? V : __builtin_nan("");
            a.press[b] = P;
        }
        const double rate = st_d[4];
        baro = !closing && rate > 0.0;
        if (baro) {
            double de = -((rate * (st_d[3] - P)) * dt);
            if (s.kT > 0.0) {
                double xi[3];
                md_noise(0u, s.step, MD_TAG_BAROSTAT, s.seed, xi);
                de = __builtin_fma(sqrt(2.0 * s.kT * rate * dt / V), xi[0], de);
            }
            strained = !has_volume || !(fabs(de) <= max_strain);                    // (a NaN does not pass)
            if (!strained) sc = exp(de / 3.0);
        }
        if (!closing && !strained) {                           // uniform
            // pass 1b: the number of free atoms whose candidate, from s x and v / s, is not within max_disp of s x
            for (int64_t i = n0 + threadIdx.x; i < n1; i += MD_THREADS) {
                if (fixed && fixed[i]) continue;
                const double m = a.mass[i];
                double v[3], xs[3], vs[3], xn[3], vn[3];
                md_closed_velocity(a, s, i, m, v);
                md_start(a, i, baro, sc, v, xs, vs);
                acc[1] += md_candidate(a, s, i, (uint32_t)(i - n0), m, xs, vs, xn, vn) <= max_disp ? 0.0 : 1.0;
            }
            block_reduce<1, 1>(acc + 1, red2);
        }
    }
    const bool accepted = !closing && !strained && !(acc[1] > 0.0);

    // pass 2: the velocities (and, of an accepted step, the positions); a fixed atom's velocity is written as zero, and where the
    // barostat acts its position rides with the cell
    for (int64_t i = n0 + threadIdx.x; i < n1; i += MD_THREADS) {
        double v[3] = {0.0, 0.0, 0.0};
        if (!(fixed && fixed[i])) {
            const double m = a.mass[i];
            md_closed_velocity(a, s, i, m, v);
            if (accepted) {
                double xs[3], vs[3], xn[3], vn[3];
                md_start(a, i, baro, sc, v, xs, vs);
                md_candidate(a, s, i, (uint32_t)(i - n0), m, xs, vs, xn, vn);
#pragma unroll
                for (int k = 0; k < 3; ++k) {
                    a.pos[i * 3 + k] = xn[k];
                    v[k] = vn[k];
                }
            }
        } else if (CELL && accepted && baro) {
#pragma unroll
            for (int k = 0; k < 3; ++k) a.pos[i * 3 + k] = sc * a.pos[i * 3 + k];
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) a.vel[i * 3 + k] = v[k];
    }
    if (threadIdx.x == 0) {
        a.ekin[b] = 0.5 * acc[0];
        if (accepted) {
            a.steps[b] = steps + 1;
            if (CELL && baro)
                for (int k = 0; k < 9; ++k) a.cell[b * 9 + k] = sc * C[k];
        } else {
            a.status[b] = closing ? 1 : (strained ? 3 : 2);
        }
    }
}

__global__ __launch_bounds__(MD_THREADS) void md_velocities_kernel(double* vel, const double* mass, const uint8_t* fixed,
                                                                   const int64_t* node_ptr, int64_t N, const double* kT,
                                                                   const int64_t* seed, int zero_momentum) {
#pragma clang fp contract(off)
    __shared__ double red[STRUCT_WAVES][5];
    __shared__ double st_kT;
    __shared__ int64_t st_seed;
    const int64_t b = blockIdx.x;
    int64_t n0 = node_ptr[b], n1 = node_ptr[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > N ? N : n0);
    n1 = n1 < n0 ? n0 : (n1 > N ? N : n1);
    if (threadIdx.x == 0) {
        st_kT = kT[b];
        st_seed = seed[b];
    }
    __syncthreads();
    const double kT_b = st_kT;
    const int64_t seed_b = st_seed;

    // pass 1: v = sqrt(kT / m) xi, written; acc = (sum m v | sum m, the number of free atoms)
    double acc[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
    for (int64_t i = n0 + threadIdx.x; i < n1; i += MD_THREADS) {
        double v[3] = {0.0, 0.0, 0.0};
        if (!(fixed && fixed[i])) {
            const double m = mass[i], sigma = sqrt(kT_b / m);
            double xi[3];
            md_noise((uint32_t)(i - n0), 0u, MD_TAG_VELOCITIES, seed_b, xi);
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                v[k] = sigma * xi[k];
                acc[k] += m * v[k];
            }
            acc[3] += m;
            acc[4] += 1.0;
        }
#pragma unroll
        for (int k = 0; k < 3; ++k) vel[i * 3 + k] = v[k];
    }
    block_reduce<5, 5>(acc, red);
    if (!zero_momentum || !(acc[4] >= 2.0)) return;            // uniform
    // pass 2: the centre-of-mass velocity of the free atoms leaves; every lane re-reads the rows it wrote itself
    const double cx = acc[0] / acc[3], cy = acc[1] / acc[3], cz = acc[2] / acc[3];
    for (int64_t i = n0 + threadIdx.x; i < n1; i += MD_THREADS) {
        if (fixed && fixed[i]) continue;
        vel[i * 3 + 0] = vel[i * 3 + 0] - cx;
        vel[i * 3 + 1] = vel[i * 3 + 1] - cy;
        vel[i * 3 + 2] = vel[i * 3 + 2] - cz;
    }
}

// an empty batch (N == 0) launches nothing and has no grid to overflow
int md_check(const char* fn, int64_t N, int64_t B) {
    MDL_REQUIRE(N >= 0 && B >= 0, MDL_E_ARG, "%s: bad N=%lld B=%lld", fn, (long long)N, (long long)B);
    MDL_REQUIRE(N == 0 || B < (1ll << 31), MDL_E_UNSUPP, "%s: B=%lld structures overflow the grid", fn, (long long)B);
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

extern "C" int mdl_md_step(double* pos, double* vel, const float* force, const double* mass, const uint8_t* fixed,
                           const int64_t* node_ptr, int64_t N, int64_t B, const double* dt, const double* gamma, const double* kT,
                           const int64_t* seed, const int32_t* n_steps, int32_t* steps, int32_t* status, double* ekin, double max_disp,
                           double* cell, const float* strain_grad, const double* pressure, const double* baro_rate, double* volume,
                           double* press, double max_strain, mdlStream_t stream) {
    using namespace mdl;
    if (const int err = md_check("mdl_md_step", N, B)) return err;
    MDL_REQUIRE(max_disp > 0.0, MDL_E_ARG, "mdl_md_step: max_disp must be > 0 (got %g)", max_disp);
    if (cell) {                                                // the cell mode
        MDL_REQUIRE(max_strain > 0.0, MDL_E_ARG, "mdl_md_step: cell mode: max_strain must be > 0 (got %g)", max_strain);
        MDL_REQUIRE(strain_grad && pressure && baro_rate && volume && press, MDL_E_ARG, "mdl_md_step: cell mode: null pointer");
    }
    if (B == 0 || N == 0) return MDL_OK;
    MDL_REQUIRE(pos && vel && force && mass && node_ptr && dt && gamma && kT && seed && n_steps && steps && status && ekin, MDL_E_ARG,
                "mdl_md_step: null pointer");
    const MdArgs a = {pos,  vel,  force,       mass,     fixed,     node_ptr, N,    dt, gamma, kT, seed, n_steps, steps, status,
                      ekin, cell, strain_grad, pressure, baro_rate, volume,   press};
    if (cell)
        hipLaunchKernelGGL(md_step_kernel<true>, dim3((unsigned)B), dim3(MD_THREADS), 0, (hipStream_t)stream, a, max_disp, max_strain);
    else
        hipLaunchKernelGGL(md_step_kernel<false>, dim3((unsigned)B), dim3(MD_THREADS), 0, (hipStream_t)stream, a, max_disp, 0.0);
    return check_launch("mdl_md_step");
}

extern "C" int mdl_md_velocities(double* vel, const double* mass, const uint8_t* fixed, const int64_t* node_ptr, int64_t N, int64_t B,
                                 const double* kT, const int64_t* seed, int zero_momentum, mdlStream_t stream) {
    using namespace mdl;
    if (const int err = md_check("mdl_md_velocities", N, B)) return err;
    if (B == 0 || N == 0) return MDL_OK;
    MDL_REQUIRE(vel && mass && node_ptr && kT && seed, MDL_E_ARG, "mdl_md_velocities: null pointer");
    hipLaunchKernelGGL(md_velocities_kernel, dim3((unsigned)B), dim3(MD_THREADS), 0, (hipStream_t)stream, vel, mass, fixed, node_ptr, N,
                       kT, seed, zero_momentum);
    return check_launch("mdl_md_velocities");
}
