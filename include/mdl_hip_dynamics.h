/* mdl_hip_dynamics.h — C ABI of the time-correlation layer of libmdl_hip.so (csrc/vacf.hip).
 *
 * A third layer, behind the engine of include/mdl_hip.h and beside the analysis layer of include/mdl_hip_analysis.h: it CONSUMES what
 * lies on the device in front of an integrator launch (velocities, the forces just evaluated, masses, time steps, the integrator's
 * step and status words) and feeds nothing back.  No reference counterpart.  The conventions are the analysis header's: every
 * pointer is a device pointer, the caller owns every buffer, nothing is allocated or synchronised, every call is asynchronous on
 * `stream`, 0 = ok, negative = MDL_E_* with the text in the engine's last-error string.  B == 0 or N == 0 returns 0 without a launch.
 * All arithmetic is fp64, contraction off, every multiply-add written out.  No atomics.
 */
#ifndef MDL_HIP_DYNAMICS_H
#define MDL_HIP_DYNAMICS_H

#include "mdl_hip_analysis.h"

#ifdef __cplusplus
extern "C" {
#endif

/* ---- The velocity AT the evaluated positions, one launch -----------------------------------------------------------
 * Between two launches of the integrator `vel` lacks the closing half kick of the step: the integrator applies it at the start of
 * its next call, from the force evaluated in between.  This entry point restates that one statement (item 2 of the integrator's
 * update in include/mdl_hip.h) on the same operands, so the on-step velocity exists without a change to the engine.
 *   vel [N, 3] fp64;  force [N, 3] fp32, at the positions vel belongs to;  mass [N] fp64;  fixed [N] uint8 or NULL;  node_ptr [B + 1]
 *   int64 (clamped to [0, N]);  dt [B] fp64;  steps [B] int32, status [B] int32 or NULL: the integrator's words, as they are IN FRONT
 *   of its launch;  read.  out [N, 3] fp64: written.
 * One workgroup of 256 lanes per structure.  Structure b is skipped — its rows of out keep their bits — if status[b] != 0 or if it
 * has no atoms.  Else, per atom i of b and component k, with h = 0.5 * dt[b]:
 *   fixed[i] != 0:  out = 0
 *   steps[b] > 0:   out = fma(h, (double)force / mass[i], vel)
 *   steps[b] == 0:  out = vel            (no step made yet: vel is the velocity at these positions)
 * This is bit for bit what the integrator's next launch takes for its kinetic energy, and what its closing call stores.  In the
 * cell mode it is the velocity BEFORE the barostat's 1 / s scaling of that step.
 * MDL_E_ARG: negative sizes, null pointers.  MDL_E_UNSUPP: B >= 2^31. */
int mdl_md_onstep_velocity(const double* vel, const float* force, const double* mass, const uint8_t* fixed, const int64_t* node_ptr,
                           const double* dt, const int32_t* steps, const int32_t* status, int64_t N, int64_t B, double* out,
                           mdlStream_t stream);

/* ---- Velocity autocorrelation against a ring of stored origins, one launch per sampled frame ----------------------
 *   v [N, 3], origins [K, N, 3] fp64;  lag [K] int32, written by the host: slot k holds the velocities of lag[k] samples ago, < 0 (or
 *   >= n_lags): the slot is skipped;  mass [N] fp64;  types [N] int32;  fixed [N] uint8 or NULL;  node_ptr;  status or NULL;  read.
 *   vacf_sum [B, 2, T, n_lags] fp64, vacf_count [B, n_lags] int64: accumulated in place.
 * One workgroup of 256 lanes per (structure b, live slot k); status[b] != 0 and empty structures are skipped.  Over the free atoms,
 * v0 the slot's origin:
 *   1. remove_com != 0: U = sum m v / sum m and U0 = sum m v0 / sum m, the velocity of the centre of mass now and at the origin (each
 *      0 without free atoms);  u = v - U, u0 = v0 - U0.  Else u = v, u0 = v0.
 *   2. per atom d = fma(u_z, u0_z, fma(u_x, u0_x, u_y * u0_y));  per type t: plane 0: S_t = sum d, plane 1: M_t = sum m * d, over the
 *      free atoms of type t (an atom whose type is outside 0 .. T - 1 is left out).
 *   3. lane 0: vacf_sum[b, 0, t, lag[k]] += S_t and vacf_sum[b, 1, t, lag[k]] += M_t for every t, vacf_count[b, lag[k]] += 1.
 * Live slots must have distinct lags (the caller's schedule): then one workgroup touches an accumulator word per launch.  Sums by
 * wave shuffles, then the waves through LDS in wave order, lanes striding from the structure's first atom: the same bits on every
 * run, alone and in any batch.  MDL_E_ARG: K < 0, n_lags < 1, T < 1, negative sizes, null pointers.  MDL_E_UNSUPP: T >
 * MDL_MSD_MAX_TYPES, K > 65535, B >= 2^31. */
int mdl_vacf_accumulate(const double* v, const double* origins, const int32_t* lag, const double* mass, const int32_t* types,
                        const uint8_t* fixed, const int64_t* node_ptr, const int32_t* status, int64_t N, int64_t B, int32_t K, int32_t T,
                        int32_t n_lags, int remove_com, double* vacf_sum, int64_t* vacf_count, mdlStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MDL_HIP_DYNAMICS_H */
