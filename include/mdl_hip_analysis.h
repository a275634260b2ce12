/* mdl_hip_analysis.h — C ABI of the trajectory-analysis layer of libmdl_hip.so (csrc/observe.hip).
 *
 * A separate layer behind the engine of include/mdl_hip.h: it CONSUMES trajectories (positions, cells and the integrator's status
 * words) and feeds nothing back.  No reference counterpart: the reference moves no atoms.  The conventions are the engine's: every
 * pointer is a device pointer, the caller owns every buffer, nothing is allocated or synchronised, every call is asynchronous on
 * `stream`, 0 = ok, negative = MDL_E_* with the text in the engine's last-error string.  B == 0 or N == 0 returns 0 without a launch.
 * All geometry is fp64, contraction off, every multiply-add written out.
 */
#ifndef MDL_HIP_ANALYSIS_H
#define MDL_HIP_ANALYSIS_H

#include "mdl_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* the pair histogram of a workgroup lives in LDS: T (T + 1) / 2 * nbins 32-bit counters, at most this many (32 KiB of the 64 KiB a
 * workgroup may have without asking; with the two staged tiles of 256 atoms, 14 KiB, three workgroups fit a CU's 160 KiB).
 * T <= 4 with nbins <= 512 is 5120. */
#define MDL_RDF_MAX_COUNTERS 8192
/* the largest number of periodic images per axis and direction, ceil(r_max / h_k).  One pass of a tile of 256 atoms i over a tile
 * of 256 atoms j adds at most 256 * 256 * (2 * 16 + 1)^3 = 2 355 167 232 < 2^32 to one LDS counter, and the counters are flushed to
 * the 64-bit histogram behind every such pass: no counter can overflow, whatever the structure. */
#define MDL_RDF_MAX_IMAGES 16
#define MDL_MSD_MAX_TYPES 64
/* bits of flag[b] */
#define MDL_RDF_NO_VOLUME 1  /* a periodic axis without extent: the cell (or its periodic part) has no volume, or is not finite */
#define MDL_RDF_TOO_MANY_IMAGES 2 /* ceil(r_max / h_k) > MDL_RDF_MAX_IMAGES along a periodic axis */
#define MDL_RDF_BAD_TYPE 4   /* an atom's type is outside 0 .. T - 1: the atom is left out, the structure is still counted */
#define MDL_RDF_TOO_LARGE 8  /* the structure has more than max_atoms atoms */

/* ---- Radial distribution: one partial pair histogram per structure, one launch per sampled frame ----------------
 *   pos [N, 3] fp64, unwrapped;  types [N] int32 in 0 .. T - 1;  node_ptr [B + 1] int64 (clamped to [0, N]);  cell [B, 3, 3] fp64, rows
 *   are lattice vectors;  pbc [B] int32, bit k: axis k is periodic;  status [B] int32 or NULL;  read.
 *   max_atoms: an upper bound of the atoms of one structure (it sizes the grid; the caller knows it from node_ptr).
 *   hist [B, P, nbins] int64 with P = T (T + 1) / 2, pair (a <= b) at a T - a (a - 1) / 2 + (b - a);  frames [B] int64;  vol_sum [B]
 *   fp64;  flag [B] int32;  accumulated in place.
 * Structure b is skipped — nothing of it is written — if status[b] != 0 or if it has no atoms.  Else, with C its cell:
 *   1. the lattice: the periodic rows of C; a non-periodic axis gets a unit row orthogonal to the periodic ones (its own row of C is
 *      not looked at), so slabs and wires need no vacuum cell.  If !(|det| > 0) of that lattice: flag |= MDL_RDF_NO_VOLUME.  Heights
 *      h_k = 1 / |column k of the inverse|, m_k = ceil(r_max / h_k) on periodic axes, 0 elsewhere; !(m_k <= MDL_RDF_MAX_IMAGES):
 *      flag |= MDL_RDF_TOO_MANY_IMAGES.  More atoms than max_atoms: flag |= MDL_RDF_TOO_LARGE.  A structure flagged with one of
 *      these three is not counted: hist, frames and vol_sum keep their bits.
 *   2. every ordered pair (i, j, n) of atoms i, j of b and integer image vectors n with (j, n) != (i, 0): d = x_j - x_i, f = d C^-1,
 *      s_k = rint(f_k) on periodic axes, d0 = d - s C (so the fractional coordinates of d0 are in [-1/2, 1/2] wherever the atoms
 *      sit), and for every |n_k| <= m_k: r = |d0 + n C|.  r < r_max: hist[b, pair(type_i, type_j), (int)(r * (nbins / r_max))] += 1
 *      (a bin index that rounding takes to nbins counts in the last bin).  Every image within r_max has |f_k + n_k| h_k <= r, so it
 *      is inside the range and is counted once, whatever the skew of the cell; i == j with n != 0 counts.
 *   3. frames[b] += 1 and vol_sum[b] += |det C| (of the cell as given; 0 where no axis is periodic), by one lane of one workgroup.
 * Grid: (structure, tiles of 256 atoms i); atoms j pass through LDS in tiles of 256, the work items of a pass are (i, j, n_0);
 * counts go to a histogram in LDS with 32-bit integer LDS atomics and from there to hist with 64-bit integer global atomics.
 * Integer sums: the result does not depend on the order, so it is bitwise repeatable and the same alone and in any batch.
 * MDL_E_ARG: !(r_max > 0), nbins < 1, T < 1, negative sizes, null pointers.  MDL_E_UNSUPP: P * nbins > MDL_RDF_MAX_COUNTERS, more
 * than 65535 tiles. */
int mdl_rdf_accumulate(const double* pos, const int32_t* types, const int64_t* node_ptr, const double* cell, const int32_t* pbc,
                       const int32_t* status, int64_t N, int64_t B, int64_t max_atoms, double r_max, int32_t nbins, int32_t T,
                       int64_t* hist, int64_t* frames, double* vol_sum, int32_t* flag, mdlStream_t stream);

/* ---- Mean-squared displacement against a ring of stored origins, one launch per sampled frame --------------------
 *   pos [N, 3], origins [K, N, 3] fp64;  lag [K] int32, written by the host: slot k holds the positions of lag[k] samples ago, < 0
 *   (or >= n_lags): the slot is skipped;  mass [N] fp64;  types [N] int32;  fixed [N] uint8 or NULL;  node_ptr;  status or NULL;  read.
 *   msd_sum [B, T, n_lags] fp64, msd_count [B, n_lags] int64: accumulated in place.
 * One workgroup of 256 lanes per (structure b, live slot k); status[b] != 0 and empty structures are skipped.  Over the free atoms:
 *   1. remove_com != 0: D = sum m (x - x0) / sum m, the displacement of the centre of mass since that origin (0 without free atoms);
 *      else D = 0.
 *   2. per type t: S_t = sum over the free atoms of type t of |x - x0 - D|^2.
 *   3. lane 0: msd_sum[b, t, lag[k]] += S_t for every t, msd_count[b, lag[k]] += 1.
 * Live slots must have distinct lags (the caller's schedule): then one workgroup touches an accumulator word per launch, and there
 * are no atomics.  Sums by wave shuffles, then the waves through LDS in wave order: the same bits on every run, alone and in any
 * batch.  MDL_E_ARG: K < 0, n_lags < 1, T < 1, negative sizes, null pointers.  MDL_E_UNSUPP: T > MDL_MSD_MAX_TYPES, K > 65535. */
int mdl_msd_accumulate(const double* pos, const double* origins, const int32_t* lag, const double* mass, const int32_t* types,
                       const uint8_t* fixed, const int64_t* node_ptr, const int32_t* status, int64_t N, int64_t B, int32_t K, int32_t T,
                       int32_t n_lags, int remove_com, double* msd_sum, int64_t* msd_count, mdlStream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MDL_HIP_ANALYSIS_H */
