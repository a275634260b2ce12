/* mdl_hip_scattering.h — C ABI of the reciprocal-space layer of libmdl_hip.so (csrc/sq.hip).
 *
 * A fourth layer, behind the engine of include/mdl_hip.h and beside the analysis layer (include/mdl_hip_analysis.h) and the
 * time-correlation layer (include/mdl_hip_dynamics.h): it CONSUMES positions, cells, pbc and the integrator's status words and feeds
 * nothing back.  No reference counterpart.  The conventions are those of the other two: every pointer is a device pointer, the
 * caller owns every buffer, nothing is allocated or synchronised, every call is asynchronous on `stream`, 0 = ok, negative =
 * MDL_E_* with the text in the engine's last-error string.  B == 0, N == 0 or Q == 0 returns 0 without a launch.  All arithmetic is
 * fp64, contraction off, every multiply-add written out: a * b + c below is a rounded product and a rounded sum, sums are taken
 * left to right as written.  No floating-point atomics.
 */
#ifndef MDL_HIP_SCATTERING_H
#define MDL_HIP_SCATTERING_H

#include "mdl_hip_dynamics.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the per-type accumulators of a workgroup of mdl_density_modes live in LDS, [T][256] complex fp64: 4 KiB per type, 32 KiB at this
 * many types.  With the staged chunk of 256 atoms (three fractional coordinates and a type each, 7 KiB) a workgroup then has
 * 39 KiB and four workgroups (16 waves) fit a CU's 160 KiB; at T <= 3 the LDS allows eight and more. */
#define MDL_SQ_MAX_TYPES 8
/* bits of flag[b] */
#define MDL_SQ_NOT_PERIODIC 1 /* (pbc & 7) != 7: a structure that is not periodic along all three axes has no reciprocal lattice */
#define MDL_SQ_NO_VOLUME 2    /* !(|det C| > 0), |det C| not finite, or an element of C not finite */
#define MDL_SQ_BAD_TYPE 4     /* an atom's type is outside 0 .. T - 1: the atom is left out, the structure is still counted */
#define MDL_SQ_FATAL 3        /* NOT_PERIODIC | NO_VOLUME: a structure that has one of these is out of every later launch */

/* ---- Density modes of every type at a list of reciprocal-lattice vectors, one launch per sampled frame ------------
 *   pos [N, 3] fp64, unwrapped;  types [N] int32;  node_ptr [B + 1] int64 (clamped to [0, N]);  cell [B, 3, 3] fp64, rows are lattice
 *   vectors;  pbc [B] int32, bit k: axis k is periodic;  status [B] int32 or NULL;  qvec [Q, 3] int32: integer triples n, shared by
 *   the whole batch — the wave vector of structure b is q = 2 pi n C^-T, so that q . x = 2 pi n . f with f the fractional
 *   coordinates;  read.
 *   rho [B, T, Q, 2] fp64 (re, im): written.  frames [B] int64, cell_sum [B, 9] fp64, flag [B] int32: accumulated in place.
 * Structure b is skipped — nothing of it is written, rho[b] keeps its bits — if status[b] != 0, if it has no atoms, or if
 * flag[b] & MDL_SQ_FATAL is set on entry.  Else, with C = cell[b] (C[3 r + c], row r):
 *   1. (pbc[b] & 7) != 7: bits |= MDL_SQ_NOT_PERIODIC.  With
 *          adj = { C4 C8 - C5 C7,  C2 C7 - C1 C8,  C1 C5 - C2 C4,
 *                  C5 C6 - C3 C8,  C0 C8 - C2 C6,  C2 C3 - C0 C5,
 *                  C3 C7 - C4 C6,  C1 C6 - C0 C7,  C0 C4 - C1 C3 }   and   det = (C0 adj0 + C1 adj3) + C2 adj6:
 *      !(|det| > 0), !(|det| < inf) or an element of C not finite: bits |= MDL_SQ_NO_VOLUME.  If bits != 0: flag[b] |= bits, and
 *      nothing else of b is written in this launch (it is not counted).  Flags are sticky: the structure stays out of every later
 *      launch of both entry points.
 *   2. Cinv[k] = adj[k] / det, formed once per workgroup from the same numbers in every lane.  Per atom i with x = pos[i]:
 *          f_k = (x_0 Cinv[k] + x_1 Cinv[3 + k]) + x_2 Cinv[6 + k]                                      k = 0, 1, 2
 *   3. an atom whose type is outside 0 .. T - 1 is left out of every sum and sets flag[b] |= MDL_SQ_BAD_TYPE (not fatal).
 *   4. for every q with n = qvec[q] (converted to fp64 exactly) and every type t, over the atoms i of type t in ASCENDING atom
 *      index, starting from (+0, +0):
 *          phi = (n_0 f_0 + n_1 f_1) + n_2 f_2;   r = phi - rint(phi);   (s, c) = sincospi(2 r)  — sin and cos of pi * (2 r)
 *          re = re + c;   im = im - s
 *      rho[b, t, q] = (re, im): the sum of exp(-i q . x_i), a plain sequential sum.  Fixed atoms scatter like any other.
 *   5. frames[b] += 1 and cell_sum[b, k] += C[k] for k = 0 .. 8, by one lane of the workgroup of the first q-tile.
 * Grid: (structure, tiles of 256 q-vectors), one q per lane; the atoms pass through LDS in chunks of 256, every loading lane forms
 * its atom's f once, every lane then walks the chunk with broadcast LDS reads and adds into its own column of the [T][256] complex
 * accumulators in LDS: no cross-lane reduction, no atomics, a fixed order — a structure's rho has the same bits on every run,
 * alone and in any batch.  Cost: (atoms of b) * Q sincospi.
 * MDL_E_ARG: negative sizes, T < 1, null pointers.  MDL_E_UNSUPP: T > MDL_SQ_MAX_TYPES, more than 65535 q-tiles, B >= 2^31. */
int mdl_density_modes(const double* pos, const int32_t* types, const int64_t* node_ptr, const double* cell, const int32_t* pbc,
                      const int32_t* status, const int32_t* qvec, int64_t N, int64_t B, int32_t Q, int32_t T, double* rho,
                      int64_t* frames, double* cell_sum, int32_t* flag, mdlStream_t stream);

/* ---- Partial structure factors and intermediate scattering functions against a ring of stored modes, one launch per frame ----
 *   rho [B, T, Q, 2] fp64, the modes of this frame;  origins [K, B, T, Q, 2] fp64, the ring (the caller stores an origin with a
 *   plain copy of rho);  lag [K] int32, written by the host: slot k holds the modes of lag[k] samples ago, < 0 or >= n_lags: the slot
 *   is skipped;  flag [B] int32, as mdl_density_modes left it;  status [B] int32 or NULL;  node_ptr [B + 1] int64 (clamped to
 *   [0, N]);  read.
 *   s_sum [B, P, Q] fp64, f_sum [B, P, n_lags, Q] fp64, f_count [B, n_lags] int64: accumulated in place.  P = T (T + 1) / 2, the pair
 *   (a <= c) at a T - a (a - 1) / 2 + (c - a), as in mdl_rdf_accumulate.
 * Structure b is skipped if status[b] != 0, if flag[b] & MDL_SQ_FATAL, or if it has no atoms.  Work items are (b, slot k or the
 * "self" slot, pair, q).  With R = rho[b] and O = origins[k, b] (the self slot: O = R), for the pair (a, c) and every q:
 *       w = 0.5 * ((R[a].re O[c].re + R[a].im O[c].im) + (R[c].re O[a].re + R[c].im O[a].im))
 *   slot k:  f_sum[b, pair, lag[k], q] += w        self:  s_sum[b, pair, q] += w
 * the real part of rho_a conj(rho0_c), symmetrised in the pair.  The self slot makes S(q) a sample of EVERY frame, whatever the
 * spacing of the origins.  One lane of a (b, live k) adds 1 to f_count[b, lag[k]].  Live slots must have distinct lags (the
 * caller's schedule): then one lane touches an accumulator word per launch — no atomics, and since every word is a fixed
 * expression of rounded products and sums the result is reproducible to the bit.
 * K == 0 is legal and gives S only (origins, lag, f_sum and f_count may then be NULL).
 * MDL_E_ARG: K < 0, n_lags < 1, T < 1, negative sizes, null pointers.  MDL_E_UNSUPP: T > MDL_SQ_MAX_TYPES, K > 65535, more than 65535
 * q-tiles, B >= 2^31. */
int mdl_sq_accumulate(const double* rho, const double* origins, const int32_t* lag, const int32_t* flag, const int32_t* status,
                      const int64_t* node_ptr, int64_t N, int64_t B, int32_t K, int32_t T, int32_t Q, int32_t n_lags, double* s_sum,
                      double* f_sum, int64_t* f_count, mdlStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MDL_HIP_SCATTERING_H */
