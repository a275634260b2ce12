"""CPU checks of the reciprocal-space layer (forces.Scatter, ops.density_modes, ops.sq_accumulate; csrc/sq.hip,
include/mdl_hip_scattering.h), and the fp64 numpy restatements that tests/test_gpu_sq.py compares the kernels with:

  density_modes_reference   the density modes of every type at integer triples n, statement by statement and in the summation order
                            of the header, and beside every word of rho a rounding bound (derived below).
  sq_accumulate_reference   the products of the modes with themselves and with a ring of origins: a fixed expression of rounded
                            products and sums per word, so the kernel's BITS can be asked for.
  density_modes_exact       the same sums in high precision (mpmath at 40 digits where it can be imported, numpy.longdouble else),
                            from the same fp64 inputs: what both the restatement and the kernel are held against.

The restatements are checked here against cases with known answers — a simple-cubic lattice in a cubic and in a sheared cell (Bragg
peaks of height N, nothing in between), n = 0, a pair of atoms, shifts by whole lattice vectors — and against the high-precision
restatement on the inputs of the GPU tests, which this file owns (gpu_inputs)."""
import functools
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import test_observe_host as toh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -53                                                 # the unit roundoff of fp64
# The accuracy of the device's sincospi is not stated in the ROCm documents shipped with the toolchain (searched for "sincospi":
# only the declaration __ocml_sincospi_f64 in hip/amd_detail/math_fwd.h).  Measured on the MI355X through ops.density_modes itself:
# one atom in a unit cell at x = (r, 0, 0) and n = (1, 0, 0) make every statement in front of sincospi exact, so rho = (cospi(2 r),
# -sinpi(2 r)) of the device; over the 636 846 reduced phases r of both frames of gpu_inputs() (every counted structure, all 257
# vectors) and 17 special ones (0, +-1/2, +-1/4, +-1/8, 3/8, 1/3, 1/6, 1/12, +-1e-300, +-2^-60, neighbours of 1/2 and 1/4) the largest
# absolute deviation from mpmath at 40 digits was 9.62e-17 for the cosine and 9.29e-17 for the sine (one run; numpy's cos / sin of
# pi * (2 r), the restatement's stand-in, was off by 3.48e-16 at worst on the same phases).
SINCOSPI_MEASURED = 9.62e-17
# what a term's (cos, sin) may be off by: four times the measured deviation of the device, plus what the restatement's own stand-in
# for sincospi, numpy's cos / sin of the ROUNDED product pi * (2 r), |2 r| <= 1, may be off by: pi u from the argument and u from
# the function
E_SINCOS = 4.0 * SINCOSPI_MEASURED + (math.pi + 1.0) * U


def adjugate(C):
    """the adjugate and the determinant of a row-major 3x3 as the header states them, and first-order bounds of their rounding errors
    (Python floats are fp64 and nothing is contracted)"""
    C = [float(v) for v in np.asarray(C, np.float64).reshape(9)]
    terms = ((4, 8, 5, 7), (2, 7, 1, 8), (1, 5, 2, 4), (5, 6, 3, 8), (0, 8, 2, 6), (2, 3, 0, 5), (3, 7, 4, 6), (1, 6, 0, 7), (0, 4, 1, 3))
    adj = [C[i] * C[j] - C[k] * C[l] for i, j, k, l in terms]
    e_adj = [2.0 * U * (abs(C[i] * C[j]) + abs(C[k] * C[l])) for i, j, k, l in terms]
    det = (C[0] * adj[0] + C[1] * adj[3]) + C[2] * adj[6]
    e_det = sum(abs(C[j]) * e_adj[3 * j] for j in range(3)) + 3.0 * U * sum(abs(C[j] * adj[3 * j]) for j in range(3))
    return C, adj, e_adj, det, e_det


def density_modes_reference(pos, types, node_ptr, cell, pbc, status, qvec, T, acc=None):
    """mdl_density_modes in numpy, one frame: (rho [B, T, Q, 2], frames [B], cell_sum [B, 9], flag [B], bound [B, T, Q, 2]).  acc: the
    first four arrays to start from (copied; rho of a skipped structure keeps what it has), or None for zeros.

    The bound of a word of rho, first order in u = 2^-53, against the exact sums of the same fp64 inputs.  A rounded product or sum
    is off by at most u times its magnitude, so
      adj_k = p - m (two products, a difference):             e_adj_k <= 2 u (|p| + |m|)
      det = (C0 adj0 + C1 adj3) + C2 adj6:                    e_det   <= sum_j |C_j| e_adj_3j + 3 u sum_j |C_j adj_3j|
      Cinv_k = adj_k / det:                                   e_inv_k <= e_adj_k / |det| + |adj_k| e_det / det^2 + u |Cinv_k|
      f_k = (x0 Cinv_k + x1 Cinv_3+k) + x2 Cinv_6+k:          e_f_k   <= sum_r |x_r| e_inv_3r+k + 3 u sum_r |x_r Cinv_3r+k|
      phi = (n0 f0 + n1 f1) + n2 f2:                          e_phi   <= sum_k |n_k| e_f_k + 3 u sum_k |n_k f_k|
    (three products and two sums of at most the sum of the magnitudes: 3 u).  phi - rint(phi) and the doubling are exact.  cos and
    sin of 2 pi phi change by at most 2 pi e_phi, and sincospi itself adds E_SINCOS (above): a term is off by at most
    2 pi e_phi + E_SINCOS.  The sequential sum S_1, S_2, ... of a (type, q) adds u |S_j| per addition.  Hence
      bound = sum over the atoms of the type of (2 pi e_phi + E_SINCOS)  +  u sum_j |S_j|
    — 2 pi sum_k |n_k| times the error of f_k, plus the error of sincospi, plus the additions.  It is derived from the statements
    and the measured accuracy of sincospi alone, never from the kernel's rho."""
    pos, cell, qvec = np.asarray(pos, np.float64), np.asarray(cell, np.float64), np.asarray(qvec)
    B, Q = len(node_ptr) - 1, len(qvec)
    if acc is None:
        rho, frames, cell_sum, flag = np.zeros((B, T, Q, 2)), np.zeros(B, np.int64), np.zeros((B, 9)), np.zeros(B, np.int32)
    else:
        rho, frames, cell_sum, flag = (np.array(x) for x in acc)
    bound = np.zeros((B, T, Q, 2))
    n = qvec.astype(np.float64)
    for b in range(B):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        if e == a or (status is not None and status[b] != 0) or flag[b] & 3:
            continue
        C, adj, e_adj, det, e_det = adjugate(cell[b])
        bits = (1 if (int(pbc[b]) & 7) != 7 else 0) | (2 if not (np.isfinite(C).all() and abs(det) > 0.0 and abs(det) < math.inf) else 0)
        if bits:
            flag[b] |= bits
            continue
        inv = [v / det for v in adj]
        e_inv = [e_adj[k] / abs(det) + abs(adj[k]) * e_det / (det * det) + U * abs(inv[k]) for k in range(9)]
        x, t = pos[a:e], np.asarray(types[a:e])
        f = np.stack([(x[:, 0] * inv[k] + x[:, 1] * inv[3 + k]) + x[:, 2] * inv[6 + k] for k in range(3)], 1)
        e_f = np.stack([sum(np.abs(x[:, r]) * e_inv[3 * r + k] for r in range(3)) + 3.0 * U * sum(np.abs(x[:, r] * inv[3 * r + k]) for r in range(3))
                        for k in range(3)], 1)
        phi = (n[None, :, 0] * f[:, None, 0] + n[None, :, 1] * f[:, None, 1]) + n[None, :, 2] * f[:, None, 2]         # [atoms, Q]
        e_phi = np.abs(n) @ e_f.T                                                                                  # [Q, atoms]
        e_phi = e_phi.T + 3.0 * U * sum(np.abs(n[None, :, k] * f[:, None, k]) for k in range(3))
        r = phi - np.rint(phi)
        c, s = np.cos(np.pi * (2.0 * r)), np.sin(np.pi * (2.0 * r))
        e_term = 2.0 * np.pi * e_phi + E_SINCOS
        if ((t < 0) | (t >= T)).any():
            flag[b] |= 4
        for ty in range(T):
            sel = t == ty
            if not sel.any():
                rho[b, ty] = 0.0
                continue
            re, im = np.cumsum(c[sel], 0), np.cumsum(-s[sel], 0)                  # sequential, in ascending atom index
            rho[b, ty, :, 0], rho[b, ty, :, 1] = re[-1], im[-1]
            bound[b, ty, :, 0] = e_term[sel].sum(0) + U * np.abs(re).sum(0)
            bound[b, ty, :, 1] = e_term[sel].sum(0) + U * np.abs(im).sum(0)
        frames[b] += 1
        cell_sum[b] = cell_sum[b] + np.asarray(C)
    return rho, frames, cell_sum, flag, bound


def sq_accumulate_reference(rho, origins, lag, flag, status, node_ptr, T, n_lags, acc=None):
    """mdl_sq_accumulate in numpy, one frame: (s_sum [B, P, Q], f_sum [B, P, n_lags, Q], f_count [B, n_lags]) — every word the header's
    expression, product by product, so the kernel's bits can be asked for.  origins [K, B, T, Q, 2] and lag [K] (K may be 0).  acc: the
    three arrays to add to (copied), or None for zeros."""
    rho = np.asarray(rho, np.float64)
    B, Q, P = len(node_ptr) - 1, rho.shape[2], T * (T + 1) // 2
    ss, fs, fc = ((np.zeros((B, P, Q)), np.zeros((B, P, n_lags, Q)), np.zeros((B, n_lags), np.int64)) if acc is None
                  else tuple(np.array(x) for x in acc))
    for b in range(B):
        if node_ptr[b + 1] == node_ptr[b] or (status is not None and status[b] != 0) or flag[b] & 3:
            continue
        R = rho[b]
        for k in [None] + [k for k, lg in enumerate(lag) if 0 <= lg < n_lags]:
            O = R if k is None else np.asarray(origins[k][b], np.float64)
            pair = 0
            for ta in range(T):
                for tc in range(ta, T):
                    w = 0.5 * ((R[ta, :, 0] * O[tc, :, 0] + R[ta, :, 1] * O[tc, :, 1]) + (R[tc, :, 0] * O[ta, :, 0] + R[tc, :, 1] * O[ta, :, 1]))
                    if k is None:
                        ss[b, pair] = ss[b, pair] + w
                    else:
                        fs[b, pair, lag[k]] = fs[b, pair, lag[k]] + w
                    pair += 1
            if k is not None:
                fc[b, lag[k]] += 1
    return ss, fs, fc


def _high_precision():
    """(number, cos, sin, pi, nearest integer) of the high-precision arithmetic there is"""
    try:
        import mpmath
        mp = mpmath.mp.clone()
        mp.dps = 40
        return mp.mpf, mp.cos, mp.sin, mp.pi, mp.nint
    except ImportError:
        L = np.longdouble
        return L, np.cos, np.sin, L("3.14159265358979323846264338327950288419716939937510"), np.rint


def density_modes_exact(pos, types, cell, qvec, T):
    """rho [T, Q, 2] of ONE periodic structure in high precision from the same fp64 inputs, rounded to fp64 at the end"""
    num, cos, sin, pi, nint = _high_precision()
    C = [num(float(v)) for v in np.asarray(cell, np.float64).reshape(9)]
    adj = [C[4] * C[8] - C[5] * C[7], C[2] * C[7] - C[1] * C[8], C[1] * C[5] - C[2] * C[4], C[5] * C[6] - C[3] * C[8], C[0] * C[8] - C[2] * C[6],
           C[2] * C[3] - C[0] * C[5], C[3] * C[7] - C[4] * C[6], C[1] * C[6] - C[0] * C[7], C[0] * C[4] - C[1] * C[3]]
    det = C[0] * adj[0] + C[1] * adj[3] + C[2] * adj[6]
    inv = [v / det for v in adj]
    zero = num(0.0)
    acc = [[[zero, zero] for _ in qvec] for _ in range(T)]
    for x, t in zip(np.asarray(pos, np.float64), types):
        if not 0 <= t < T:
            continue
        x = [num(float(v)) for v in x]
        f = [x[0] * inv[k] + x[1] * inv[3 + k] + x[2] * inv[6 + k] for k in range(3)]
        for j, n in enumerate(qvec):
            phi = int(n[0]) * f[0] + int(n[1]) * f[1] + int(n[2]) * f[2]
            ang = 2 * pi * (phi - nint(phi))
            acc[t][j][0] += cos(ang)
            acc[t][j][1] -= sin(ang)
    return np.array([[[float(v) for v in w] for w in row] for row in acc], np.float64).reshape(T, len(qvec), 2)


# ---------------------------------------------------------------------------------------------
# the inputs of tests/test_gpu_sq.py
# ---------------------------------------------------------------------------------------------
# one atom, a pair, a wave - 1, exactly one wave, a wave + 1, the chunk of 256, the chunk + 1, two chunks + 1, and the roles
SIZES = [1, 2, 63, 64, 65, 256, 257, 513, 0, 7, 9, 11, 5]
ONE, PAIR, WAVE_LESS, WAVE, WAVE_MORE, CHUNK, CHUNK_MORE, BIG, EMPTY, STOPPED, OPEN, BAD, SINGULAR = range(13)
Q_MAX, N_COMPONENT = 257, 8


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    """(node_ptr, cell, pbc, status, qvec [257, 3], pos, pos2): skewed triclinic cells, positions unwrapped out to +-3 cells, integer
    triples with negative and zero components up to |n_k| = 8; a stopped structure, one that is periodic along two axes only, one
    whose cell has a zero row; pos2 a second frame"""
    rng = np.random.default_rng(61)
    node_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    N, B = int(node_ptr[-1]), len(SIZES)
    cell = rng.uniform(-2.0, 2.0, (B, 3, 3))
    cell[:, range(3), range(3)] = rng.uniform(5.0, 9.0, (B, 3))                     # (diagonally dominant: a volume well away from 0)
    frac = rng.uniform(-3.0, 3.0, (N, 3))
    pos = np.concatenate([frac[a:e] @ cell[b] for b, (a, e) in enumerate(zip(node_ptr[:-1], node_ptr[1:]))])
    cell[SINGULAR, 2] = 0.0
    pbc, status = np.full(B, 7, np.int32), np.zeros(B, np.int32)
    pbc[OPEN], status[STOPPED] = 3, 2
    qvec = rng.integers(-N_COMPONENT, N_COMPONENT + 1, (Q_MAX, 3)).astype(np.int32)
    qvec[0], qvec[1], qvec[2], qvec[3], qvec[-1] = (8, -8, 0), (0, 0, 0), (-8, 8, 8), (0, 0, -1), (8, 8, -8)
    pos2 = pos + 0.05 * rng.normal(size=pos.shape)
    return node_ptr, cell, pbc, status, qvec, pos, pos2


@functools.lru_cache(maxsize=None)
def gpu_types(T):
    """types of gpu_inputs() in 0 .. T - 1, but for ONE atom of the structure BAD, whose type is T"""
    node_ptr = gpu_inputs()[0]
    types = np.random.default_rng(70 + T).integers(0, T, int(node_ptr[-1])).astype(np.int32)
    types[node_ptr[BAD] + 4] = T
    return types


@functools.lru_cache(maxsize=None)
def gpu_reference(T, Q, frame=0):
    """density_modes_reference of one frame of gpu_inputs() from zeros"""
    node_ptr, cell, pbc, status, qvec, pos, pos2 = gpu_inputs()
    return density_modes_reference(pos2 if frame else pos, gpu_types(T), node_ptr, cell, pbc, status, qvec[:Q], T)


def observations(qvec, sq_sum, sq_frames, cell_sum, type_totals, fqt_sum=None, fqt_count=None):
    """a forces.Observations around host arrays: its helpers are torch arithmetic and run anywhere"""
    from matdeeplearn_amd import forces
    t = lambda a, d: None if a is None else torch.from_numpy(np.ascontiguousarray(np.asarray(a, d)))
    o = forces.Observations.__new__(forces.Observations)
    o.qvec, o.sq_sum, o.sq_frames, o.cell_sum = t(qvec, np.int32), t(sq_sum, np.float64), t(sq_frames, np.int64), t(cell_sum, np.float64)
    o.type_totals, o.fqt_sum, o.fqt_count = t(type_totals, np.int64), t(fqt_sum, np.float64), t(fqt_count, np.int64)
    return o


# ---------------------------------------------------------------------------------------------
# 1. the surface
# ---------------------------------------------------------------------------------------------
def test_scattering_header_and_prototype_table_agree_and_the_other_layers_are_what_they_were():
    from matdeeplearn_amd import _build, _lib, ops
    header = open(os.path.join(ROOT, "include", "mdl_hip_scattering.h")).read()
    declared = toh._declared("mdl_hip_scattering.h")
    assert declared == set(_lib.SCATTERING_PROTOTYPES) == {"mdl_density_modes", "mdl_sq_accumulate"}
    assert not declared & (set(_lib.PROTOTYPES) | set(_lib.ANALYSIS_PROTOTYPES) | set(_lib.DYNAMICS_PROTOTYPES))
    assert set(_lib.DYNAMICS_PROTOTYPES) == toh._declared("mdl_hip_dynamics.h") and set(_lib.ANALYSIS_PROTOTYPES) == toh._declared("mdl_hip_analysis.h")
    assert len(toh._declared("mdl_hip.h")) == 84 == len(_lib.PROTOTYPES)
    assert '#include "mdl_hip_dynamics.h"' in header
    for name, (res, args) in _lib.SCATTERING_PROTOTYPES.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(proto.split(",")) == len(args) == 16, name
    if os.path.exists(_build.LIB):
        handle = _lib.lib()
        for name in declared:
            assert hasattr(handle, name), name
            assert getattr(handle, name).argtypes == _lib.SCATTERING_PROTOTYPES[name][1]
    assert _build.FILE_FLAGS["sq.hip"] == ["-ffp-contract=off"] and "mdl_hip_scattering.h" in inspect.getsource(_build._deps_mtime)
    for macro, value in (("MDL_SQ_MAX_TYPES", ops.SQ_MAX_TYPES), ("MDL_SQ_NOT_PERIODIC", ops.SQ_NOT_PERIODIC), ("MDL_SQ_NO_VOLUME", ops.SQ_NO_VOLUME),
                         ("MDL_SQ_BAD_TYPE", ops.SQ_BAD_TYPE), ("MDL_SQ_FATAL", ops.SQ_FATAL)):
        assert re.search(r"#define %s %d\b" % (macro, value), header), macro
    assert ops.SQ_FATAL == ops.SQ_NOT_PERIODIC | ops.SQ_NO_VOLUME and not ops.SQ_FATAL & ops.SQ_BAD_TYPE
    # the LDS budget the header states: [T][256] complex accumulators and the staged chunk; four workgroups in a CU's 160 KiB
    lds = ops.SQ_MAX_TYPES * 256 * 16 + 256 * (3 * 8 + 4)
    assert ops.SQ_MAX_TYPES * 256 * 16 == 32 * 1024 and 4 * (lds + 256) <= 160 * 1024 < 5 * lds
    assert ops.SqState.__slots__ == ("types", "node_ptr", "n_types", "qvec", "rho", "frames", "cell_sum", "flag", "sq_sum", "n_lags", "origins",
                                     "fqt_sum", "fqt_count")


def test_scatter_is_a_correlate_and_the_pinned_signatures_stand():
    from matdeeplearn_amd import forces, ops
    assert issubclass(forces.Scatter, forces.Correlate)
    assert str(inspect.signature(forces.Scatter)) == "(every=1, skip=0, rdf=None, msd=None, frames_every=0, types=None, vacf=None, sq=None)"
    assert str(inspect.signature(forces.Correlate)) == "(every=1, skip=0, rdf=None, msd=None, frames_every=0, types=None, vacf=None)"
    assert str(inspect.signature(forces.sample)) == "(model, structs, dist_range, masses, dt, steps, observe, npt=None, **md_kwargs)"
    assert str(inspect.signature(ops.sq_numbers)) == "(who, n_types=None, sq=None, n_structs=None)"
    assert str(inspect.signature(ops.sq_state)) == "(types, node_ptr, n_types=None, sq=None, device=None)"
    assert str(inspect.signature(ops.density_modes)) == "(pos, cell, pbc, state, status=None)"
    assert str(inspect.signature(ops.sq_accumulate)) == "(lag, state, status=None)"
    new = ("qvec", "sq_sum", "sq_frames", "sq_flag", "cell_sum", "fqt_sum", "fqt_count")
    params = inspect.signature(forces.Observations).parameters
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY and params[k].default is None for k in new)
    assert [k for k in params if k not in new] == ["state", "species", "type_counts", "type_totals", "frames_pos", "frames_cell", "frames_step",
                                                   "lag_time", "pbc", "vacf_state", "frames_vel"]
    for k in ("q", "q_norm", "sq", "sq_radial", "fqt"):
        assert callable(getattr(forces.Observations, k))
    for k in ("F_s", "X-ray", "neutron", "not periodic"):                       # what is out of scope is said
        assert k in forces.Scatter.__doc__, k
    s = forces.Scatter()
    assert (s.every, s.skip, s.rdf, s.msd, s.frames_every, s.types, s.vacf, s.sq) == (1, 0, None, None, 0, None, None, None)
    s = forces.Scatter(every=2, vacf=dict(n_lags=8), sq=dict(n_max=1, fqt=dict(n_lags=6, origin_every=4)))
    assert s.vacf["n_lags"] == 8 and s.sq["fqt"] == dict(n_lags=6, origin_every=4, n_origins=2) and s.sq["max_bytes"] == 2 ** 30
    assert s.sq["q"].shape == (13, 3) and s.sq["q"].dtype == np.int32 and sorted(s.sq) == ["fqt", "max_bytes", "q"]
    assert forces.Scatter(sq=s.sq).sq["fqt"] == s.sq["fqt"]                      # what it returns is a request itself
    s = forces.Scatter(sq=dict(q=[[0, 0, 0], [1, -2, 3]], max_bytes=100))
    assert s.sq["q"].tolist() == [[0, 0, 0], [1, -2, 3]] and s.sq["fqt"] is None and s.sq["max_bytes"] == 100
    # only a Scatter that asks gets a state for it: a plain Observe or Correlate has none
    from matdeeplearn_amd.process import graph as pg
    p = pg.pack_structures(toh._structs())
    asked = lambda req: forces._Observer(req, p, 6).sq
    assert asked(forces.Observe(frames_every=1)) is None and asked(forces.Correlate(vacf=dict(n_lags=2))) is None and asked(forces.Scatter()) is None
    assert asked(forces.Scatter(sq=dict(n_max=2)))["q"].shape == (62, 3)


def test_the_half_space_has_every_vector_once_in_lexicographic_order():
    from matdeeplearn_amd import ops
    for n_max in (1, 2, 4):
        q = ops.sq_half_space(n_max)
        assert q.dtype == np.int32 and q.shape == (((2 * n_max + 1) ** 3 - 1) // 2, 3) and np.abs(q).max() == n_max
        rows = [tuple(r) for r in q.tolist()]
        assert rows == sorted(rows) and len(set(rows)) == len(rows)
        for r in rows:                                          # the first non-zero component is positive
            assert [v for v in r if v != 0][0] > 0
        both = set(rows) | {tuple(-v for v in r) for r in rows}
        assert len(both) == 2 * len(rows) == (2 * n_max + 1) ** 3 - 1 and (0, 0, 0) not in both
    assert ops.sq_half_space(1).tolist() == [[0, 0, 1], [0, 1, -1], [0, 1, 0], [0, 1, 1], [1, -1, -1], [1, -1, 0], [1, -1, 1], [1, 0, -1], [1, 0, 0],
                                             [1, 0, 1], [1, 1, -1], [1, 1, 0], [1, 1, 1]]
    assert len(ops.sq_half_space(4)) == 364


def test_argument_errors_raise_before_a_device_is_needed():
    from matdeeplearn_amd import forces, ops
    E = ops.MdlError
    for sq, msg in ((dict(), "exactly one of q and n_max"), (dict(q=[[1, 0, 0]], n_max=1), "exactly one of q and n_max"),
                    (dict(n_max=1, lags=3), "sq must be dict"), ([1, 2], "sq must be dict"), (dict(n_max=0), "n_max must be an integer >= 1"),
                    (dict(n_max=1.5), "n_max must be an integer >= 1"), (dict(n_max=True), "n_max must be an integer >= 1"),
                    (dict(q=[1, 0, 0]), r"q must be a \[Q, 3\] integer array"), (dict(q=[[1.0, 0.0, 0.0]]), r"q must be a \[Q, 3\] integer array"),
                    (dict(q=np.zeros((2, 2), np.int64)), r"q must be a \[Q, 3\] integer array"), (dict(q=[[2 ** 31, 0, 0]]), "fit 32 bits"),
                    (dict(n_max=1, fqt=dict(n_lags=0)), "sq: fqt: n_lags must be >= 1"), (dict(n_max=1, fqt=dict(origin_every=2)), "fqt must be dict"),
                    (dict(n_max=1, fqt=dict(n_lags=2, remove_com=True)), "fqt must be dict"), (dict(n_max=1, fqt=3), "fqt must be dict"),
                    (dict(n_max=1, fqt=dict(n_lags=4, origin_every=0)), "sq: fqt: origin_every must be >= 1"),
                    (dict(n_max=1, fqt=dict(n_lags=4, n_origins=65536)), "sq: fqt: n_origins must be in 1"), (dict(n_max=1, max_bytes=-1), "max_bytes")):
        with pytest.raises(E, match=msg):
            forces.Scatter(sq=sq)
        with pytest.raises(E, match=msg):
            ops.sq_state([0, 0, 1], [0, 3], sq=sq, device="cpu")
    with pytest.raises(E, match="every must be >= 1"):
        forces.Scatter(every=0, sq=dict(n_max=1))
    with pytest.raises(E, match="vacf: n_lags"):
        forces.Scatter(vacf=dict(n_lags=0), sq=dict(n_max=1))
    # the byte budget, before anything is allocated: 8 B P n_lags Q + 16 K B T Q
    B, T, Q, n_lags, K = 2, 2, 13, 6, 3
    need = 8 * B * 3 * n_lags * Q + 16 * K * B * T * Q
    fqt = dict(n_lags=n_lags, origin_every=2)
    assert ops.sq_numbers("x", T, dict(n_max=1, fqt=fqt, max_bytes=need), B)["fqt"]["n_origins"] == K
    with pytest.raises(E, match=r"8·B·P·n_lags·Q \+ 16·K·B·T·Q = %d bytes.*max_bytes = %d" % (need, need - 1)):
        ops.sq_numbers("x", T, dict(n_max=1, fqt=fqt, max_bytes=need - 1), B)
    with pytest.raises(E, match="8·B·P·n_lags·Q"):
        ops.sq_state([0, 1, 1, 0], [0, 2, 4], sq=dict(n_max=1, fqt=fqt, max_bytes=need - 1), device="cpu")
    assert ops.sq_numbers("x", T, dict(n_max=1, max_bytes=0), B)["fqt"] is None          # S(q) alone is not held against it
    big = dict(n_max=4, fqt=dict(n_lags=64, origin_every=4))                             # 4096 structures of three types: 5.7 GB
    with pytest.raises(E, match="more than max_bytes = %d" % 2 ** 30):
        ops.sq_numbers("x", 3, big, 4096)
    # what needs the structures: forces.sample raises before it looks at the model (None here) or at a device
    structs, masses = toh._structs(), np.ones(5)
    run = lambda o, **kw: forces.sample(None, structs, (0.0, 8.0), masses, 1.0, 4, o, **kw)
    with pytest.raises(E, match="sq: at most 8 types"):
        run(forces.Scatter(sq=dict(n_max=1), types=[0, 1, 2, 3, 8]))
    with pytest.raises(E, match="8·B·P·n_lags·Q"):
        run(forces.Scatter(sq=dict(n_max=2, fqt=dict(n_lags=4), max_bytes=1000)))
    with pytest.raises(E, match="energy_and_forces"):                            # past the observer's checks: the model is looked at
        run(forces.Scatter(sq=dict(n_max=1)))
    # ops.sq_state and the two calls
    with pytest.raises(E, match="sq must be dict"):
        ops.sq_state([0, 1], [0, 2], device="cpu")
    with pytest.raises(E, match=r"types must be in 0 \.\. 1"):
        ops.sq_state([0, 1, 2], [0, 3], n_types=2, sq=dict(n_max=1), device="cpu")
    with pytest.raises(E, match="node_ptr must start at 0"):
        ops.sq_state([0, 1, 2, 3], [0, 3], sq=dict(n_max=1), device="cpu")
    with pytest.raises(E, match="at most 8 types"):
        ops.sq_state([0, 8], [0, 2], sq=dict(n_max=1), device="cpu")
    st = ops.sq_state([0, 1, 1], [0, 1, 3], sq=dict(n_max=1, fqt=dict(n_lags=4, origin_every=2)), device="cpu")
    assert (st.n_types, st.n_lags) == (2, 4) and st.pair_index(1, 0) == 1 and st.pair_index(1, 1) == 2
    assert [tuple(getattr(st, k).shape) for k in ("qvec", "rho", "frames", "cell_sum", "flag", "sq_sum", "origins", "fqt_sum", "fqt_count")] == [
        (13, 3), (2, 2, 13, 2), (2,), (2, 9), (2,), (2, 3, 13), (2, 2, 2, 13, 2), (2, 3, 4, 13), (2, 4)]
    plain = ops.sq_state([0, 1, 1], [0, 1, 3], sq=dict(q=np.array([[0, 0, 0]])), device="cpu")
    assert plain.fqt_sum is None and plain.fqt_count is None and tuple(plain.origins.shape) == (0, 2, 2, 1, 2) and plain.n_lags == 0
    pos, cell, pbc = torch.zeros(3, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64).repeat(2, 1, 1), torch.full((2,), 7, dtype=torch.int32)
    with pytest.raises(E):                                                       # tensors on the host: no kernel to run them
        ops.density_modes(pos, cell, pbc, st)
    with pytest.raises(E):
        ops.sq_accumulate(torch.zeros(2, dtype=torch.int32), st)
    for bad in (dict(pos=pos[:2]), dict(pos=pos.float()), dict(cell=cell[:1]), dict(pbc=pbc.long()), dict(state=None), dict(status=torch.zeros(3, dtype=torch.int32))):
        a = dict(dict(pos=pos, cell=cell, pbc=pbc, state=st, status=None), **bad)
        with pytest.raises(E):
            ops.density_modes(a["pos"], a["cell"], a["pbc"], a["state"], a["status"])
    with pytest.raises(E, match="lag must be None"):
        ops.sq_accumulate(torch.zeros(2, dtype=torch.int32), plain)
    with pytest.raises(E, match=r"lag must be a contiguous \[K\] int32"):
        ops.sq_accumulate(torch.zeros(2, dtype=torch.int64), st)


# ---------------------------------------------------------------------------------------------
# 2. known answers
# ---------------------------------------------------------------------------------------------
L, A = 4, 1.5                                                   # i / 4 and 1.5 i are exact, and so are the products below
SHEAR = np.array([[1.0, 0.0, 0.0], [0.25, 1.0, 0.0], [0.5, -0.75, 1.0]])


def _lattice(cell):
    frac = np.array([(i, j, k) for i in range(L) for j in range(L) for k in range(L)], np.float64) / L
    return frac @ cell                                           # exact: small dyadic rationals


@pytest.mark.parametrize("sheared", [False, True])
def test_a_simple_cubic_lattice_has_bragg_peaks_of_height_n_and_nothing_between(sheared):
    cell = L * A * (SHEAR if sheared else np.eye(3))
    pos = _lattice(cell)
    N = L ** 3
    qvec = np.array([(i, j, k) for i in range(-5, 6) for j in range(-5, 6) for k in range(-5, 6)], np.int32)
    rho, frames, cell_sum, flag, bound = density_modes_reference(pos, np.zeros(N, np.int32), [0, N], cell[None], [7], None, qvec, 1)
    assert frames.tolist() == [1] and flag.tolist() == [0] and np.array_equal(cell_sum[0], cell.reshape(9))
    peak = (qvec % L == 0).all(1)
    assert peak.sum() == 27 and bound.max() < 1e-11 and bound.min() > 0
    want = np.zeros((len(qvec), 2))
    want[peak, 0] = N
    err = np.abs(rho[0, 0] - want)
    print("simple cubic, sheared %s: largest |rho - known| %.3e, largest ratio to the bound %.3f" % (sheared, err.max(), (err / bound[0, 0]).max()))
    assert (err <= bound[0, 0]).all()


def test_n_zero_counts_the_atoms_of_every_type_exactly():
    node_ptr, cell, pbc, status, qvec, pos, _ = gpu_inputs()
    for T in (1, 3, 8):
        rho = gpu_reference(T, 4)[0]
        types = gpu_types(T)
        assert qvec[1].tolist() == [0, 0, 0]
        for b in (ONE, PAIR, WAVE_MORE, BIG, BAD):
            t = types[node_ptr[b]:node_ptr[b + 1]]
            assert rho[b, :, 1, 0].tolist() == [float((t == ty).sum()) for ty in range(T)] and not rho[b, :, 1, 1].any()
        assert rho[BAD, :, 1, 0].sum() == SIZES[BAD] - 1         # the atom of the unknown type is left out


def test_a_pair_of_atoms_interferes_as_two_plus_two_cos():
    cell = 4.0 * np.eye(3)                                       # Cinv = 1 / 4 and f = x / 4 exactly
    rng = np.random.default_rng(5)
    pos = rng.integers(-2048, 2048, (2, 3)) / 64.0
    qvec = rng.integers(-8, 9, (64, 3)).astype(np.int32)
    rho, _, _, _, bound = density_modes_reference(pos, [0, 0], [0, 2], cell[None], [7], None, qvec, 1)
    d = (pos[1] - pos[0]) / 4.0                                  # exact
    phase = qvec.astype(np.float64) @ d                          # exact: a few bits each
    want = 2.0 + 2.0 * np.cos(2.0 * np.pi * (phase - np.rint(phase)))
    re, im, (b_re, b_im) = rho[0, 0, :, 0], rho[0, 0, :, 1], (bound[0, 0, :, 0], bound[0, 0, :, 1])
    tol = 2.0 * (np.abs(re) * b_re + np.abs(im) * b_im) + b_re ** 2 + b_im ** 2 + 8.0 * U * (2.0 * np.pi + 4.0)
    assert (np.abs(re * re + im * im - want) <= tol).all() and tol.max() < 1e-10 and want.min() < 1.0 < 3.0 < want.max()


def test_shifting_atoms_by_whole_lattice_vectors_leaves_rho_alone():
    cell = L * A * SHEAR
    rng = np.random.default_rng(6)
    N = 40
    pos = rng.integers(-4096, 4096, (N, 3)) / 256.0
    shifted = pos + rng.integers(-3, 4, (N, 3)).astype(np.float64) @ cell             # exact: dyadic rationals of a few bits
    types = rng.integers(0, 3, N)
    qvec = rng.integers(-8, 9, (50, 3)).astype(np.int32)
    one = density_modes_reference(pos, types, [0, N], cell[None], [7], None, qvec, 3)
    two = density_modes_reference(shifted, types, [0, N], cell[None], [7], None, qvec, 3)
    err, tol = np.abs(one[0] - two[0]), one[4] + two[4]
    assert (err <= tol).all() and err.max() > 0 and tol.max() < 1e-10


def test_the_flags_are_sticky_and_a_flagged_or_stopped_structure_keeps_what_it_has():
    node_ptr, cell, pbc, status, qvec, pos, pos2 = gpu_inputs()
    T, Q, B = 3, 5, len(SIZES)
    rng = np.random.default_rng(7)
    base = (rng.normal(size=(B, T, Q, 2)), rng.integers(1, 9, B), rng.normal(size=(B, 9)), np.zeros(B, np.int32))
    first = density_modes_reference(pos, gpu_types(T), node_ptr, cell, pbc, status, qvec[:Q], T, base)
    assert first[3].tolist() == [0] * 10 + [1, 4, 2]
    for b in (EMPTY, STOPPED, OPEN, SINGULAR):
        assert all(np.array_equal(first[k][b], base[k][b]) for k in range(3))
    counted = [b for b in range(B) if b not in (EMPTY, STOPPED, OPEN, SINGULAR)]
    assert np.array_equal(first[1][counted], base[1][counted] + 1) and np.array_equal(first[2][counted], base[2][counted] + cell[counted].reshape(-1, 9))
    # healed: the flags keep the two structures out all the same
    second = density_modes_reference(pos2, gpu_types(T), node_ptr, np.where(np.arange(B)[:, None, None] == SINGULAR, np.eye(3), cell),
                                     np.full(B, 7, np.int32), status, qvec[:Q], T, first[:4])
    assert second[3].tolist() == first[3].tolist()
    for b in (OPEN, SINGULAR):
        assert all(np.array_equal(second[k][b], base[k][b]) for k in range(3))
    assert np.array_equal(second[1][counted], base[1][counted] + 2)
    # a cell that is not finite, or without volume in any other way
    for bad in (np.diag([1.0, np.inf, 1.0]), np.diag([1.0, np.nan, 1.0]), np.zeros((3, 3)), np.array([[1.0, 2, 3], [2, 4, 6], [0, 0, 1]]),
                np.diag([1e200, 1e200, 1e200])):
        assert density_modes_reference(np.zeros((1, 3)), [0], [0, 1], bad[None], [7], None, qvec[:2], 1)[3].tolist() == [2]


def test_the_restatement_stays_within_its_own_bound_of_high_precision_on_the_gpu_inputs():
    """the condition that the GPU tests' inputs are fair: at these cells, positions and integers the fp64 restatement itself is
    within the bound it hands the kernel.  Every counted structure, T = 3, the vectors with the largest components and a few others."""
    node_ptr, cell, pbc, status, qvec, pos, _ = gpu_inputs()
    T = 3
    pick = [0, 1, 2, 3, 100, 255, 256]
    rho, _, _, flag, bound = gpu_reference(T, Q_MAX)
    types = gpu_types(T)
    worst = 0.0
    for b in (ONE, PAIR, WAVE_LESS, WAVE, WAVE_MORE, CHUNK, CHUNK_MORE, BIG, BAD):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        exact = density_modes_exact(pos[a:e], types[a:e], cell[b], qvec[pick], T)
        err, lim = np.abs(rho[b][:, pick] - exact), bound[b][:, pick] + U * np.abs(exact)      # (+ the rounding of `exact` to fp64)
        assert (err <= lim).all(), (b, float((err / lim).max()))
        worst = max(worst, float((err[lim > 0] / lim[lim > 0]).max()))
    print("the restatement against high precision: at worst %.3f of its bound; the largest bound %.3e" % (worst, bound.max()))
    assert 0 < worst and bound.max() < 1e-9


def test_sq_accumulate_reference_is_the_symmetrised_real_part_and_skips_what_it_must():
    rng = np.random.default_rng(8)
    B, T, Q, K, n_lags = 4, 3, 7, 3, 4
    node_ptr = [0, 2, 2, 5, 6]                                  # structure 1 is empty
    rho, origins = rng.normal(size=(B, T, Q, 2)), rng.normal(size=(K, B, T, Q, 2))
    flag, status = np.array([0, 0, 4, 2], np.int32), np.array([0, 0, 0, 0], np.int32)        # a bad type is not fatal; no volume is
    ss, fs, fc = sq_accumulate_reference(rho, origins, [2, -1, 4], flag, status, node_ptr, T, n_lags)
    z, z0 = rho[..., 0] + 1j * rho[..., 1], origins[..., 0] + 1j * origins[..., 1]
    pair = 0
    for a in range(T):
        for c in range(a, T):
            for b in (0, 2):
                want_s = 0.5 * (z[b, a] * z[b, c].conj() + z[b, c] * z[b, a].conj()).real
                want_f = 0.5 * (z[b, a] * z0[0, b, c].conj() + z[b, c] * z0[0, b, a].conj()).real
                assert np.allclose(ss[b, pair], want_s, rtol=0, atol=1e-14) and np.allclose(fs[b, pair, 2], want_f, rtol=0, atol=1e-14)
            pair += 1
    assert fc.tolist() == [[0, 0, 1, 0], [0, 0, 0, 0], [0, 0, 1, 0], [0, 0, 0, 0]]
    assert not ss[[1, 3]].any() and not fs[[1, 3]].any() and not fs[:, :, [0, 1, 3]].any()
    assert np.array_equal(ss[0, 0], rho[0, 0, :, 0] * rho[0, 0, :, 0] + rho[0, 0, :, 1] * rho[0, 0, :, 1])           # 0.5 * (x + x) = x, exactly
    # stopped, and K = 0
    ss2, fs2, fc2 = sq_accumulate_reference(rho, origins[:0], [], flag, np.array([0, 0, 3, 0], np.int32), node_ptr, T, n_lags, (ss, fs, fc))
    assert np.array_equal(ss2[0], ss[0] + ss[0]) and np.array_equal(ss2[2], ss[2]) and np.array_equal(fs2, fs) and np.array_equal(fc2, fc)


# ---------------------------------------------------------------------------------------------
# 3. Observations on hand-made accumulators
# ---------------------------------------------------------------------------------------------
def test_observations_normalise_the_sums_and_say_nan_where_there_is_nothing():
    from matdeeplearn_amd import forces, ops
    cell = np.array([[4.0, 0.0, 0.0], [1.0, 5.0, 0.0], [0.5, -1.0, 8.0]])
    qvec = np.array([[1, 0, 0], [0, 1, 0], [0, 0, 1], [1, -2, 3], [2, 0, 0]], np.int32)
    B, T, Q, P, n_lags = 3, 2, 5, 3, 3
    frames = np.array([4, 0, 2])
    totals = np.array([[3, 2], [3, 2], [5, 0]])                 # structure 1 has no counted frame, structure 2 no atom of type 1
    cell_sum = np.stack([4 * cell.reshape(9), np.zeros(9), 2 * (2.0 * cell).reshape(9)])
    rng = np.random.default_rng(9)
    sq_sum, fqt_sum = rng.uniform(1, 2, (B, P, Q)), rng.uniform(1, 2, (B, P, n_lags, Q))
    fqt_count = np.array([[4, 2, 0], [0, 0, 0], [2, 1, 1]])
    o = observations(qvec, sq_sum, frames, cell_sum, totals, fqt_sum, fqt_count)
    q = o.q().numpy()
    want = 2.0 * np.pi * qvec @ np.linalg.inv(cell).T
    assert q.shape == (B, Q, 3) and np.allclose(q[0], want, rtol=1e-14, atol=0) and np.allclose(q[2], want / 2.0, rtol=1e-14, atol=0)
    assert np.isnan(q[1]).all() and np.allclose(q[0] @ cell.T, 2.0 * np.pi * qvec, rtol=0, atol=1e-13)          # q . a_k = 2 pi n_k
    assert np.allclose(o.q_norm().numpy()[0], np.sqrt((want ** 2).sum(1)), rtol=1e-14, atol=0)
    s01, s11, s00 = o.sq(0, 1).numpy(), o.sq(1, 1).numpy(), o.sq(0, 0).numpy()
    assert np.array_equal(o.sq(1, 0).numpy(), s01, equal_nan=True)
    assert np.allclose(s01[0], sq_sum[0, 1] / (4 * math.sqrt(6.0)), rtol=1e-15, atol=0) and np.allclose(s11[0], sq_sum[0, 2] / (4 * 2.0), rtol=1e-15, atol=0)
    assert np.allclose(s00[2], sq_sum[2, 0] / (2 * 5.0), rtol=1e-15, atol=0)
    assert np.isnan(s01[1]).all() and np.isnan(s00[1]).all() and np.isnan(s01[2]).all() and np.isnan(s11[2]).all()
    f = o.fqt(0, 1).numpy()
    assert f.shape == (B, n_lags, Q) and np.allclose(f[0, 1], fqt_sum[0, 1, 1] / (2 * math.sqrt(6.0)), rtol=1e-15, atol=0)
    assert np.isnan(f[0, 2]).all() and np.isnan(f[1]).all() and np.isnan(f[2]).all() and np.isfinite(f[0, :2]).all()
    assert np.allclose(o.fqt(0, 0).numpy()[2, 2], fqt_sum[2, 0, 2] / (1 * 5.0), rtol=1e-15, atol=0)
    # shells of |q|: the mean over the vectors in each, NaN for an empty one
    qn = o.q_norm().numpy()
    centres, radial = o.sq_radial(0, 0, 3.5, 7)
    assert np.allclose(centres.numpy(), (np.arange(7) + 0.5) * 0.5) and tuple(radial.shape) == (B, 7)
    for b in (0, 2):
        for k in range(7):
            inside = (qn[b] >= 0.5 * k) & (qn[b] < 0.5 * (k + 1))
            got = radial[b, k].item()
            assert (np.isnan(got) and not inside.any()) or np.isclose(got, s00[b][inside].mean(), rtol=1e-14, atol=0), (b, k)
    assert np.isnan(radial[1].numpy()).all() and np.isfinite(radial[0].numpy()).any() and np.isnan(radial[0].numpy()).any()
    assert (qn[0] >= 3.5).any()                                  # a vector beyond q_max is in no shell
    with pytest.raises(ops.MdlError, match="q_max > 0"):
        o.sq_radial(0, 0, 0.0, 8)
    with pytest.raises(ops.MdlError, match="types must be in 0 .. 1"):
        o.sq(0, 2)
    # a run that was not asked
    none = observations(None, None, None, None, totals)
    for call in (none.q, none.q_norm, lambda: none.sq(0, 0), lambda: none.sq_radial(0, 0, 1.0, 2), lambda: none.fqt(0, 0)):
        with pytest.raises(ops.MdlError, match="was not asked"):
            call()
    with pytest.raises(ops.MdlError, match="was not asked"):
        observations(qvec, sq_sum, frames, cell_sum, totals).fqt(0, 0)
