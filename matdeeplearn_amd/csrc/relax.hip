// relax.hip — one FIRE update (Bitzek et al., PRL 97, 170201 (2006); unit masses) of a BATCH of structures in one launch.
// No reference counterpart: the reference has no force path and no optimiser of atomic positions.
//
// ONE kernel body, fire_kernel<CELL>, instantiated twice:
//   mdl_fire_step        fire_kernel<false>: one workgroup of 256 lanes per structure, looping over the structure's atoms; all
//                   arithmetic fp64.
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
//                   Band mode (image_ptr != NULL): the band-force launch of csrc/neb.hip goes first, and the same
//                   fire_kernel<false> then moves BANDS on the force that launch wrote — a nudged-elastic-band step.
//   mdl_fire_cell_step   fire_kernel<true>: the same update over the atoms and the cell: the rows s_i (pos_i = F s_i) and the three
//                   rows of W = cf F, F the deformation gradient of the cell the relaxation started from.  Same workgroup, same
//                   sums; the 3x3 algebra (F^-1 through the adjugate, S F^-T, det cell) is done by every lane from the same nine
//                   numbers.  A step whose F' leaves |F' - I| <= max_deform is refused as a whole (done = 2) before anything of
//                   it is written.
// The bits: contraction is off in the kernel and every fused multiply-add is written out, so the source states the arithmetic
// (fp64 sqrt and / are correctly rounded, no fast-math flag is in the build).  A structure whose cell is frozen runs, in
// fire_kernel<true>, the statements that are all of fire_kernel<false>: it gets the bits of mdl_fire_step because it is that code.
#include "struct_reduce.h"

namespace mdl {
namespace {

constexpr int FIRE_THREADS = STRUCT_THREADS;                   // block_reduce (struct_reduce.h, shared with csrc/md.hip)
constexpr int FIRE_WAVES = STRUCT_WAVES;

struct FireConst {
    int32_t n_min;
    double f_inc, f_dec, alpha_start, f_alpha, dt_max, maxstep;
};

// the operands of both entry points; what only the cell's degrees of freedom need is null for mdl_fire_step and never read there
struct FireArgs {
    double *pos, *vel;
    const float* force;
    const uint8_t* fixed;
    const int64_t* node_ptr;
    int64_t N;
    const double* fmax;
    double *dt, *alpha;
    int32_t *n_pos, *steps, *done;
    float* fmax_seen;
    double *cell, *scaled, *deform, *vel_cell;
    const float* strain_grad;
    const double* cell0;
    const uint8_t* cell_free;
    const double *cell_factor, *smax;
    float* smax_seen;
};

// CELL = false: the atoms alone (include/mdl_hip.h, mdl_fire_step); free_cell is false at compile time, and no cell matrix, no
// `scaled` row and no cell pointer is touched.
// CELL = true: atoms and cell (mdl_fire_cell_step).  The atoms' passes run with the generalised force g = F^T f in the place of f
// (g = f where the cell is frozen); the three rows of W enter every sum behind the workgroup's reduction, from values every lane
// holds, and not at all where the cell is frozen.  Nothing of a structure is written before the trust region has accepted its new
// F: the velocities of a structure with a free cell are formed twice (pass 2 for the step's length, pass 3 to be stored).
// Every fma is explicit: x^2 + y^2 + z^2 is fma(z, z, fma(x, x, y y)), the mixing fma(dt, g, fma(c_f, g, c_v v)), the step
// fma(clip, dt v, pos); the F-transforms and the cell's rows are plain products and sums.
template <bool CELL>
__global__ __launch_bounds__(FIRE_THREADS) void fire_kernel(FireArgs a, FireConst c, double max_deform) {
#pragma clang fp contract(off)
    __shared__ double red1[FIRE_WAVES][4];
    __shared__ double red2[FIRE_WAVES][1];
    __shared__ double st_d[5];
    __shared__ int32_t st_i[4];
    __shared__ double m_F[9], m_S[9], m_V[9], m_C[9], m_C0[9];     // CELL only
    const int64_t b = blockIdx.x;
    int64_t n0 = a.node_ptr[b], n1 = a.node_ptr[b + 1];
    n0 = n0 < 0 ? 0 : (n0 > a.N ? a.N : n0);
    n1 = n1 < n0 ? n0 : (n1 > a.N ? a.N : n1);
    if (threadIdx.x == 0) {
        st_d[0] = a.dt[b];
        st_d[1] = a.alpha[b];
        st_d[2] = a.fmax[b];
        st_i[0] = a.n_pos[b];
        st_i[1] = a.steps[b];
        st_i[2] = a.done[b];
        if constexpr (CELL) {
            const bool fr = a.cell_free[b] != 0;
            st_d[3] = a.smax[b];
            st_d[4] = a.cell_factor[b];
            st_i[3] = fr ? 1 : 0;
            for (int k = 0; k < 9; ++k) {
                m_S[k] = (double)a.strain_grad[b * 9 + k];
                m_C[k] = a.cell[b * 9 + k];
                m_F[k] = fr ? a.deform[b * 9 + k] : (k % 4 == 0 ? 1.0 : 0.0);
                m_V[k] = fr ? a.vel_cell[b * 9 + k] : 0.0;
                m_C0[k] = fr ? a.cell0[b * 9 + k] : 0.0;
            }
        }
    }
    bool free_cell = false;
    double F[9], S[9], gW[9], V[9], Vn[9], Fn[9];                  // CELL only
    if constexpr (CELL) {
        __syncthreads();                                           // free_cell and F are needed in pass 1
        free_cell = st_i[3] != 0;
#pragma unroll
        for (int k = 0; k < 9; ++k) F[k] = m_F[k];
    }
    const uint8_t* fixed = a.fixed;
    const float* force = a.force;
    double* vel = a.vel;

    // pass 1: acc = (|g|^2, g.v, |v|^2 | max_i |f_i|^2) over the atoms; a fixed atom has f = 0 and v = 0
    double acc[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i = n0 + threadIdx.x; i < n1; i += FIRE_THREADS) {
        if (fixed && fixed[i]) continue;
        const double fx = (double)force[i * 3 + 0], fy = (double)force[i * 3 + 1], fz = (double)force[i * 3 + 2];
        const double vx = vel[i * 3 + 0], vy = vel[i * 3 + 1], vz = vel[i * 3 + 2];
        const double f2 = __builtin_fma(fz, fz, __builtin_fma(fx, fx, fy * fy));
        double gx = fx, gy = fy, gz = fz, g2 = f2;
        if (free_cell) {
            gx = F[0] * fx + F[3] * fy + F[6] * fz;
            gy = F[1] * fx + F[4] * fy + F[7] * fz;
            gz = F[2] * fx + F[5] * fy + F[8] * fz;
            g2 = __builtin_fma(gz, gz, __builtin_fma(gx, gx, gy * gy));
        }
        acc[0] += g2;
        acc[1] += __builtin_fma(vz, gz, __builtin_fma(vx, gx, vy * gy));
        acc[2] += __builtin_fma(vz, vz, __builtin_fma(vx, vx, vy * vy));
        acc[3] = f2 > acc[3] ? f2 : acc[3];
    }
    block_reduce<4, 3>(acc, red1);                             // (its barrier also publishes st_d / st_i)

    bool stress_ok = true;
    double cf = 0.0;
    if constexpr (CELL) {
        // the cell's rows: g_W = -(1 / cf) S F^-T, and the stress criterion sm = max |S| / |det cell|
        double max_s = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            S[k] = m_S[k];
            V[k] = m_V[k];
            gW[k] = 0.0;
            const double as = fabs(S[k]);
            max_s = as > max_s || as != as ? as : max_s;       // a NaN stays
        }
        double adj[9], C[9];
#pragma unroll
        for (int k = 0; k < 9; ++k) C[k] = m_C[k];
        const double det_c = adjugate3(C, adj);
        const double sm = det_c != 0.0 ? max_s / fabs(det_c) : __longlong_as_double(0x7ff8000000000000ll);
        cf = st_d[4];
        if (free_cell) {
            const double det_f = adjugate3(F, adj);
            const double scale = -(1.0 / cf);
            double gg = 0.0, gv = 0.0, vv_c = 0.0;
#pragma unroll
            for (int r = 0; r < 3; ++r)
#pragma unroll
                for (int q = 0; q < 3; ++q) {
                    const double t = S[r * 3 + 0] * (adj[q * 3 + 0] / det_f) + S[r * 3 + 1] * (adj[q * 3 + 1] / det_f) +
                                     S[r * 3 + 2] * (adj[q * 3 + 2] / det_f);
                    const double g = scale * t;
                    gW[r * 3 + q] = g;
                    gg += g * g;
                    gv += g * V[r * 3 + q];
                    vv_c += V[r * 3 + q] * V[r * 3 + q];
                }
            acc[0] += gg;
            acc[1] += gv;
            acc[2] += vv_c;
        }
        stress_ok = !free_cell || sm < st_d[3] || !(sm > 0.0);
        if (threadIdx.x == 0) a.smax_seen[b] = (float)sm;
    }
    const double ff = acc[0], P = acc[1], vv = acc[2], fm = sqrt(acc[3]);
    double dt = st_d[0], alpha = st_d[1];
    int32_t n_pos = st_i[0];
    const int32_t steps = st_i[1];
    const bool latched = st_i[2] != 0;
    const bool force_ok = fm < st_d[2] || !(fm > 0.0);
    if (threadIdx.x == 0) a.fmax_seen[b] = (float)fm;
    // every return below is uniform over the workgroup
    if constexpr (CELL)
        if (latched) return;                                   // the code (1 converged, 2 trust region) stays; without a cell it becomes 1
    if (latched || (force_ok && stress_ok)) {
        if (threadIdx.x == 0) a.done[b] = 1;
        return;
    }

    // velocity mixing: v <- c_v v + c_f g
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

    // pass 2: v <- (c_v v + c_f g) + dt g;  |dt v|^2.  Stored here only where no trust region can refuse the step
    double s2[1] = {0.0};
    for (int64_t i = n0 + threadIdx.x; i < n1; i += FIRE_THREADS) {
        double vx = 0.0, vy = 0.0, vz = 0.0;
        if (!(fixed && fixed[i])) {
            const double fx = (double)force[i * 3 + 0], fy = (double)force[i * 3 + 1], fz = (double)force[i * 3 + 2];
            double gx = fx, gy = fy, gz = fz;
            if (free_cell) {
                gx = F[0] * fx + F[3] * fy + F[6] * fz;
                gy = F[1] * fx + F[4] * fy + F[7] * fz;
                gz = F[2] * fx + F[5] * fy + F[8] * fz;
            }
            vx = __builtin_fma(dt, gx, __builtin_fma(c_f, gx, c_v * vel[i * 3 + 0]));
            vy = __builtin_fma(dt, gy, __builtin_fma(c_f, gy, c_v * vel[i * 3 + 1]));
            vz = __builtin_fma(dt, gz, __builtin_fma(c_f, gz, c_v * vel[i * 3 + 2]));
        }
        if (!free_cell) {
            vel[i * 3 + 0] = vx;
            vel[i * 3 + 1] = vy;
            vel[i * 3 + 2] = vz;
        }
        const double dx = dt * vx, dy = dt * vy, dz = dt * vz;
        s2[0] += __builtin_fma(dz, dz, __builtin_fma(dx, dx, dy * dy));
    }
    block_reduce<1, 1>(s2, red2);
    if constexpr (CELL)
        if (free_cell) {
            double s2_c = 0.0;
#pragma unroll
            for (int k = 0; k < 9; ++k) {
                Vn[k] = (c_v * V[k] + c_f * gW[k]) + dt * gW[k];
                const double d = dt * Vn[k];
                s2_c += d * d;
            }
            s2[0] += s2_c;
        }
    const double s = sqrt(s2[0]);
    const double clip = s > c.maxstep ? c.maxstep / s : 1.0;

    if (!free_cell) {
        // pass 3: pos += dt v (clipped); every lane re-reads the velocities it wrote itself.  With a cell, s follows pos (F = I)
        // (an atom's three loads stand before its stores: pos and vel are not known to be distinct, and would be read one by one)
        for (int64_t i = n0 + threadIdx.x; i < n1; i += FIRE_THREADS) {
            double px = a.pos[i * 3 + 0], py = a.pos[i * 3 + 1], pz = a.pos[i * 3 + 2];
            if (!(fixed && fixed[i])) {
                px = __builtin_fma(clip, dt * vel[i * 3 + 0], px);
                py = __builtin_fma(clip, dt * vel[i * 3 + 1], py);
                pz = __builtin_fma(clip, dt * vel[i * 3 + 2], pz);
                a.pos[i * 3 + 0] = px;
                a.pos[i * 3 + 1] = py;
                a.pos[i * 3 + 2] = pz;
            }
            if constexpr (CELL) {
                a.scaled[i * 3 + 0] = px;
                a.scaled[i * 3 + 1] = py;
                a.scaled[i * 3 + 2] = pz;
            }
        }
    } else if constexpr (CELL) {
        // W += clip dt v_W, F' = W / cf; the trust region decides before anything is written
        double dev2 = 0.0;
#pragma unroll
        for (int k = 0; k < 9; ++k) {
            Fn[k] = (cf * F[k] + (dt * Vn[k]) * clip) / cf;
            const double e = Fn[k] - (k % 4 == 0 ? 1.0 : 0.0);
            dev2 += e * e;
        }
        if (!(sqrt(dev2) <= max_deform)) {                     // too far, or a non-finite entry
            if (threadIdx.x == 0) a.done[b] = 2;
            return;
        }
        // pass 3: the velocities again (the bits of pass 2), s += clip dt v, pos = F' s for every atom
        for (int64_t i = n0 + threadIdx.x; i < n1; i += FIRE_THREADS) {
            double vx = 0.0, vy = 0.0, vz = 0.0;
            double sx = a.scaled[i * 3 + 0], sy = a.scaled[i * 3 + 1], sz = a.scaled[i * 3 + 2];
            if (!(fixed && fixed[i])) {
                const double fx = (double)force[i * 3 + 0], fy = (double)force[i * 3 + 1], fz = (double)force[i * 3 + 2];
                const double gx = F[0] * fx + F[3] * fy + F[6] * fz;
                const double gy = F[1] * fx + F[4] * fy + F[7] * fz;
                const double gz = F[2] * fx + F[5] * fy + F[8] * fz;
                vx = __builtin_fma(dt, gx, __builtin_fma(c_f, gx, c_v * vel[i * 3 + 0]));
                vy = __builtin_fma(dt, gy, __builtin_fma(c_f, gy, c_v * vel[i * 3 + 1]));
                vz = __builtin_fma(dt, gz, __builtin_fma(c_f, gz, c_v * vel[i * 3 + 2]));
                sx = __builtin_fma(clip, dt * vx, sx);
                sy = __builtin_fma(clip, dt * vy, sy);
                sz = __builtin_fma(clip, dt * vz, sz);
                a.scaled[i * 3 + 0] = sx;
                a.scaled[i * 3 + 1] = sy;
                a.scaled[i * 3 + 2] = sz;
            }
            vel[i * 3 + 0] = vx;
            vel[i * 3 + 1] = vy;
            vel[i * 3 + 2] = vz;
            a.pos[i * 3 + 0] = Fn[0] * sx + Fn[1] * sy + Fn[2] * sz;
            a.pos[i * 3 + 1] = Fn[3] * sx + Fn[4] * sy + Fn[5] * sz;
            a.pos[i * 3 + 2] = Fn[6] * sx + Fn[7] * sy + Fn[8] * sz;
        }
    }
    if (threadIdx.x == 0) {
        a.dt[b] = dt;
        a.alpha[b] = alpha;
        a.n_pos[b] = n_pos;
        a.steps[b] = steps + 1;
        if constexpr (CELL)
            if (free_cell) {
                for (int k = 0; k < 9; ++k) {
                    a.deform[b * 9 + k] = Fn[k];
                    a.vel_cell[b * 9 + k] = Vn[k];
                }
                for (int r = 0; r < 3; ++r)                    // cell = C0 F'^T: lattice vector r is F' a0_r
                    for (int q = 0; q < 3; ++q)
                        a.cell[b * 9 + r * 3 + q] = m_C0[r * 3 + 0] * Fn[q * 3 + 0] + m_C0[r * 3 + 1] * Fn[q * 3 + 1] + m_C0[r * 3 + 2] * Fn[q * 3 + 2];
            }
    }
}

// what both entry points ask of N, B and FIRE's constants; an empty batch (N == 0) launches nothing and has no grid to overflow
int fire_check(const char* fn, int64_t N, int64_t B, const FireConst& c) {
    MDL_REQUIRE(N >= 0 && B >= 0, MDL_E_ARG, "%s: bad N=%lld B=%lld", fn, (long long)N, (long long)B);
    MDL_REQUIRE(c.n_min >= 0 && c.f_inc > 0.0 && c.f_dec > 0.0 && c.f_alpha > 0.0 && c.alpha_start >= 0.0 && c.alpha_start <= 1.0 &&
                    c.dt_max > 0.0 && c.maxstep > 0.0,
                MDL_E_ARG, "%s: need n_min >= 0, f_inc, f_dec, f_alpha, dt_max, maxstep > 0 and alpha_start in [0, 1] "
                           "(got n_min=%d f_inc=%g f_dec=%g f_alpha=%g alpha_start=%g dt_max=%g maxstep=%g)",
                fn, (int)c.n_min, c.f_inc, c.f_dec, c.f_alpha, c.alpha_start, c.dt_max, c.maxstep);
    MDL_REQUIRE(N == 0 || B < (1ll << 31), MDL_E_UNSUPP, "%s: B=%lld structures overflow the grid", fn, (long long)B);
    return MDL_OK;
}

}  // namespace
}  // namespace mdl

extern "C" int mdl_fire_cell_step(double* pos, double* cell, double* scaled, double* deform, double* vel, double* vel_cell,
                                  const float* force, const float* strain_grad, const double* cell0, const uint8_t* fixed,
                                  const uint8_t* cell_free, const double* cell_factor, const int64_t* node_ptr, int64_t N, int64_t B,
                                  const double* fmax, const double* smax, double* dt, double* alpha, int32_t* n_pos, int32_t* steps,
                                  int32_t* done, float* fmax_seen, float* smax_seen, int32_t n_min, double f_inc, double f_dec,
                                  double alpha_start, double f_alpha, double dt_max, double maxstep, double max_deform,
                                  mdlStream_t stream) {
    using namespace mdl;
    const FireConst c = {n_min, f_inc, f_dec, alpha_start, f_alpha, dt_max, maxstep};
    if (const int err = fire_check("mdl_fire_cell_step", N, B, c)) return err;
    MDL_REQUIRE(max_deform > 0.0 && max_deform < 1.0, MDL_E_ARG, "mdl_fire_cell_step: max_deform must be in (0, 1) (got %g)", max_deform);
    if (B == 0 || N == 0) return MDL_OK;
    MDL_REQUIRE(pos && cell && scaled && deform && vel && vel_cell && force && strain_grad && cell0 && cell_free && cell_factor &&
                    node_ptr && fmax && smax && dt && alpha && n_pos && steps && done && fmax_seen && smax_seen,
                MDL_E_ARG, "mdl_fire_cell_step: null pointer");
    const FireArgs a = {pos,  vel,    force,  fixed,    node_ptr,    N,     fmax,      dt,          alpha, n_pos,    steps, done, fmax_seen,
                        cell, scaled, deform, vel_cell, strain_grad, cell0, cell_free, cell_factor, smax,  smax_seen};
    hipLaunchKernelGGL(fire_kernel<true>, dim3((unsigned)B), dim3(FIRE_THREADS), 0, (hipStream_t)stream, a, c, max_deform);
    return check_launch("mdl_fire_cell_step");
}

extern "C" int mdl_fire_step(double* pos, double* vel, const float* force, const uint8_t* fixed, const int64_t* node_ptr, int64_t N,
                             int64_t B, const double* fmax, double* dt, double* alpha, int32_t* n_pos, int32_t* steps, int32_t* done,
                             float* fmax_seen, int32_t n_min, double f_inc, double f_dec, double alpha_start, double f_alpha,
                             double dt_max, double maxstep, const int64_t* image_ptr, const int64_t* band_ptr, int64_t I,
                             const float* energy, const double* cell, const int32_t* pbc, const double* spring, const uint8_t* climb,
                             float* band_force, double* tangent_force, double* seg_len, int32_t* climber, mdlStream_t stream) {
    using namespace mdl;
    const FireConst c = {n_min, f_inc, f_dec, alpha_start, f_alpha, dt_max, maxstep};
    if (const int err = fire_check("mdl_fire_step", N, B, c)) return err;
    if (B == 0 || N == 0) return MDL_OK;
    MDL_REQUIRE(pos && vel && force && node_ptr && fmax && dt && alpha && n_pos && steps && done && fmax_seen, MDL_E_ARG,
                "mdl_fire_step: null pointer");
    if (image_ptr) {
        // band mode: the band force of every image first (csrc/neb.hip), then the same launch as below over the B bands on it
        const NebArgs nb = {pos,  force, fixed,  image_ptr, band_ptr,   N,             I,       B,      energy,
                            cell, pbc,   spring, climb,     band_force, tangent_force, seg_len, climber};
        if (const int err = neb_band_force("mdl_fire_step", nb, (hipStream_t)stream)) return err;
        force = band_force;
    }
    const FireArgs a = {pos, vel, force, fixed, node_ptr, N, fmax, dt, alpha, n_pos, steps, done, fmax_seen};   // the cell's fields: null
    hipLaunchKernelGGL(fire_kernel<false>, dim3((unsigned)B), dim3(FIRE_THREADS), 0, (hipStream_t)stream, a, c, 0.0);
    return check_launch("mdl_fire_step");
}
