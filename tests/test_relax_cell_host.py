"""Host side of the variable-cell relaxation tests: this file OWNS fire_cell_reference, a numpy fp64 restatement of the batched
FIRE update over atoms and cell (csrc/relax.hip mdl_fire_cell_step, ops.fire_cell_step, forces.relax_cell) as include/mdl_hip.h
states it, one structure after the other, and the fp64 reference trajectory of the oracle CGCNN at held neighbour lists that
tests/test_gpu_relax_cell.py compares forces.relax_cell with.  The upstream reference moves neither atoms nor cells.  No GPU.

Coordinates (restated): cells are row-vector matrices; C0 the cell at the start, F the deformation gradient, C = C0 F^T, atom i at
r_i = F s_i.  Degrees of freedom: the rows s_i and the three rows of W = cf F.  Generalised forces: F^T f_i on s_i and
-(1 / cf) S F^-T on W, S = dE/d eps (not divided by the volume).

TRAJ_BOUND_POS / TRAJ_BOUND_CELL, the bounds of the trajectory comparison, are the reference's own sensitivity: the same 20 steps
with every force perturbed by uniform noise of amplitude 1e-4 max|F| and every component of S by 1e-4 max|S| (the bounds
tests/test_gpu_forces and tests/test_gpu_stress put on the device values) moved the final positions by DEV_POS = 1.49e-4 A and the
final lattice vectors by DEV_CELL = 3.42e-5 A at most (measured here; atoms travel up to 1.70 A, lattice vectors 0.07 to 0.88 A);
the bounds are 10 x those, rounded up to two digits, by the project's "measured x 10" rule."""
import functools
import inspect
import os
import re

import numpy as np
import pytest
import torch

import test_gpu_forces as tgf
import test_relax_host as trh
import test_stress_host as tsh
from test_forces_host import edge_dist, edge_shifts

TRAJ_BOUND_POS = 1.5e-3       # A; 10 x DEV_POS (module docstring)
TRAJ_BOUND_CELL = 3.5e-4      # A; 10 x DEV_CELL
FIRE_CELL_CONSTANTS = dict(trh.FIRE_CONSTANTS, max_deform=0.5)
EYE = np.eye(3)


def new_cell_state(pos, cell, node_ptr, cell_free=None, cell_factor=None, dt=0.1, alpha=0.1):
    B = len(node_ptr) - 1
    st = trh.new_state(B, dt, alpha)
    st.update(scaled=np.array(pos, dtype=np.float64), deform=np.tile(EYE, (B, 1, 1)), vel_cell=np.zeros((B, 3, 3)),
              cell0=np.array(cell, dtype=np.float64), smax_seen=np.zeros(B, np.float32),
              cell_free=np.ones(B, np.uint8) if cell_free is None else (np.asarray(cell_free) != 0).astype(np.uint8),
              cell_factor=np.maximum(1, np.diff(node_ptr)).astype(np.float64) if cell_factor is None else np.array(cell_factor, dtype=np.float64))
    return st


def det3(m):
    return (m[0, 0] * (m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1]) + m[0, 1] * (m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2])
            + m[0, 2] * (m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0]))


def inv3(m):
    """the inverse through the adjugate (no pivoting, no exception: a singular or non-finite matrix gives inf / NaN entries)"""
    adj = np.array([[m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1], m[0, 2] * m[2, 1] - m[0, 1] * m[2, 2], m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                    [m[1, 2] * m[2, 0] - m[1, 0] * m[2, 2], m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], m[0, 2] * m[1, 0] - m[0, 0] * m[1, 2]],
                    [m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0], m[0, 1] * m[2, 0] - m[0, 0] * m[2, 1], m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]])
    with np.errstate(all="ignore"):
        return adj / det3(m)


def generalised_forces(f, S, F, cf):
    """(F^T f_i as rows, -(1 / cf) S F^-T)"""
    with np.errstate(all="ignore"):
        return f @ F, -(1.0 / cf) * (S @ inv3(F).T)


def fire_cell_reference(pos, cell, vel, force, strain_grad, node_ptr, state, fmax, smax, fixed=None, **constants):
    """One FIRE update of every structure over its N + 3 rows, fp64.  Returns (pos, cell, vel, state, diag) as NEW arrays (state
    holds scaled, deform, vel_cell, ...); diag[b] holds the numbers the decisions of structure b were taken from: fm, sm, P,
    abs_fv (sum over the rows of |g.v|), s and s_atoms (the step's norm with and without the cell's rows), dev (|F' - I|) and the
    branch.  A structure with a frozen cell goes through the arithmetic of test_relax_host.fire_reference, operation by operation."""
    c = dict(FIRE_CELL_CONSTANTS, **constants)
    pos, cell, vel = np.array(pos, dtype=np.float64), np.array(cell, dtype=np.float64), np.array(vel, dtype=np.float64)
    force, strain_grad = np.asarray(force, dtype=np.float64), np.asarray(strain_grad, dtype=np.float64)
    st = {k: np.array(v) for k, v in state.items()}
    B = len(node_ptr) - 1
    fmax = np.broadcast_to(np.asarray(fmax, dtype=np.float64), (B,))
    smax = np.broadcast_to(np.asarray(smax, dtype=np.float64), (B,))
    free_all = np.ones(len(pos), bool) if fixed is None else ~np.asarray(fixed).astype(bool)
    diag = []
    for b in range(B):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        free = free_all[a:e]
        fr = bool(st["cell_free"][b])
        f = np.where(free[:, None], force[a:e], 0.0)
        v = np.where(free[:, None], vel[a:e], 0.0)
        fm = float(np.sqrt((f * f).sum(1)).max()) if e > a else 0.0
        S, det_c = strain_grad[b], det3(cell[b])
        with np.errstate(all="ignore"):
            sm = float(np.abs(S).max() / abs(det_c)) if det_c != 0.0 else float("nan")
            st["fmax_seen"][b], st["smax_seen"][b] = np.float32(fm), np.float32(sm)
        d = {"fm": fm, "sm": sm, "P": 0.0, "abs_fv": 0.0, "s": 0.0, "s_atoms": 0.0, "dev": 0.0, "branch": "converged", "force_ok": None,
             "stress_ok": None}
        diag.append(d)
        if st["done"][b] != 0:                                 # latched, 1 or 2: the code stays
            d["branch"] = "latched"
            continue
        d["force_ok"] = fm < fmax[b] or not fm > 0.0
        d["stress_ok"] = (not fr) or sm < smax[b] or not sm > 0.0
        if d["force_ok"] and d["stress_ok"]:
            st["done"][b] = 1
            continue
        cf = float(st["cell_factor"][b])
        F = st["deform"][b] if fr else EYE
        if fr:
            g, gw = generalised_forces(f, S, F, cf)
            vw = st["vel_cell"][b]
        else:
            g, gw, vw = f, np.zeros((3, 3)), np.zeros((3, 3))
        dt, alpha = float(st["dt"][b]), float(st["alpha"][b])
        n_pos = int(st["n_pos"][b])
        with np.errstate(all="ignore"):
            if st["steps"][b] == 0:
                d["branch"] = "first"
            else:
                P = float((g * v).sum()) + (float((gw * vw).sum()) if fr else 0.0)
                d["P"] = P
                d["abs_fv"] = float(np.abs((g * v).sum(1)).sum()) + (float(np.abs((gw * vw).sum(1)).sum()) if fr else 0.0)
                if P > 0.0:
                    vv = (v * v).sum() + ((vw * vw).sum() if fr else 0.0)
                    gg = (g * g).sum() + ((gw * gw).sum() if fr else 0.0)
                    ratio = alpha * (np.sqrt(vv) / np.sqrt(gg))
                    v = (1.0 - alpha) * v + ratio * g
                    vw = (1.0 - alpha) * vw + ratio * gw
                    d["branch"] = "uphill-free"
                    if n_pos > c["n_min"]:
                        dt = min(dt * c["f_inc"], c["dt_max"])
                        alpha = alpha * c["f_alpha"]
                        d["branch"] = "accelerate"
                    n_pos += 1
                else:
                    v, vw = np.zeros_like(v), np.zeros((3, 3))
                    alpha, dt = c["alpha_start"], dt * c["f_dec"]
                    n_pos = 0
                    d["branch"] = "reset"
            v = v + dt * g
            vw = vw + dt * gw
            dr, drw = dt * v, dt * vw
            s_atoms = float(np.sqrt((dr * dr).sum()))
            s = float(np.sqrt((dr * dr).sum() + (drw * drw).sum())) if fr else s_atoms
            d["s"], d["s_atoms"] = s, s_atoms
            if s > c["maxstep"]:
                dr, drw = dr * (c["maxstep"] / s), drw * (c["maxstep"] / s)
            if fr:
                Fn = (cf * F + drw) / cf
                d["dev"] = float(np.sqrt(((Fn - EYE) ** 2).sum()))
                if not d["dev"] <= c["max_deform"]:            # the trust region: nothing of this update is written
                    st["done"][b] = 2
                    d["branch"] = "stopped"
                    continue
                st["scaled"][a:e] += dr
                pos[a:e] = st["scaled"][a:e] @ Fn.T
                cell[b] = st["cell0"][b] @ Fn.T
                st["deform"][b], st["vel_cell"][b] = Fn, vw
            else:
                pos[a:e] += dr
                st["scaled"][a:e] = pos[a:e]
        vel[a:e] = v
        st["dt"][b], st["alpha"][b], st["n_pos"][b] = dt, alpha, n_pos
        st["steps"][b] += 1
    return pos, cell, vel, st, diag


# ---------------------------------------------------------------------------------------------
# the periodic toy: an fcc cell, nearest-neighbour springs on a fixed edge list with image shifts
# ---------------------------------------------------------------------------------------------
A0, K_SPRING = 4.0, 1.0


@functools.lru_cache(maxsize=None)
def fcc_toy():
    """(fractional coordinates [4, 3], C0, src, tgt, integer images [E, 3]): the 48 directed nearest-neighbour bonds of the
    conventional fcc cell, every one with the lattice translation it crosses"""
    frac = np.array([[0.0, 0.0, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]])
    c0 = EYE * A0
    src, tgt, img = [], [], []
    for t in range(4):
        for s in range(4):
            for n in np.stack(np.meshgrid(*[np.arange(-1, 2)] * 3, indexing="ij"), -1).reshape(-1, 3):
                if abs(np.linalg.norm((frac[t] + n - frac[s]) @ c0) - A0 / np.sqrt(2.0)) < 1e-9:
                    src.append(s), tgt.append(t), img.append(n)
    assert len(src) == 48
    return frac, c0, np.asarray(src), np.asarray(tgt), np.asarray(img, dtype=np.float64)


def toy_energy_forces(pos, cell):
    """E = sum over the directed bonds of (k / 4) (d - d0)^2, f = -dE/dpos and S = dE/d eps (test_stress_host.strain_formula) of
    ONE toy structure at the Cartesian positions pos in the cell `cell`"""
    _, _, src, tgt, img = fcc_toy()
    s, t = torch.from_numpy(src), torch.from_numpy(tgt)
    p = torch.from_numpy(np.asarray(pos, np.float64))
    sh = torch.from_numpy(img @ np.asarray(cell, np.float64))
    d, u = tsh.unit_vectors(p, sh, s, t)
    d0 = A0 / np.sqrt(2.0)
    g = 0.5 * K_SPRING * (d - d0)
    energy = float((0.25 * K_SPRING * (d - d0) ** 2).sum())
    gu = g.unsqueeze(1) * u
    grad = torch.zeros_like(p).index_add_(0, t, gu).index_add_(0, s, -gu)
    S = tsh.strain_formula(g, d, u, torch.zeros(len(src), dtype=torch.int64), 1)[0]
    return energy, -grad.numpy(), S.numpy(), (d - d0).abs().max().item()


def strained_start(seed, strain, rattle):
    """the toy in a cell deformed by F0 = I + strain * (stretch + shear) with atoms rattled by `rattle` (fractional)"""
    frac, c0, *_ = fcc_toy()
    rng = np.random.default_rng(seed)
    f0 = EYE + strain * np.array([[1.0, 0.6, -0.3], [0.2, -0.8, 0.5], [-0.4, 0.1, 0.7]])
    cell = c0 @ f0.T
    return (frac + rattle * rng.uniform(-1, 1, frac.shape)) @ cell, cell


# 1 -------------------------------------------------------------------------------------------
def test_generalised_forces_match_central_differences_of_the_energy_in_s_and_w():
    """E(s, W) of the toy with r_i = F s_i, C = C0 F^T, F = W / cf away from I (5 % stretch and shear, atoms rattled): central
    differences (h = 1e-5: truncation ~ h^2, rounding ~ 1e-16 E / h, both below 1e-9 of the gradients) against F^T f and
    -(1 / cf) S F^-T, signs included."""
    frac, c0, *_ = fcc_toy()
    rng = np.random.default_rng(2)
    cf = 4.0
    F = EYE + 0.05 * np.array([[1.0, 0.6, -0.3], [0.2, -0.8, 0.5], [-0.4, 0.1, 0.7]])
    assert np.abs(F - F.T).max() > 0.01                                    # not symmetric: F^-T and F^-1 differ
    s0 = (frac + 0.03 * rng.uniform(-1, 1, frac.shape)) @ c0
    w0 = cf * F

    def energy(s, w):
        f_ = w / cf
        return toy_energy_forces(s @ f_.T, c0 @ f_.T)[0]

    _, f, S, _ = toy_energy_forces(s0 @ F.T, c0 @ F.T)
    g_s, g_w = generalised_forces(f, S, F, cf)
    h = 1e-5
    fd_s, fd_w = np.zeros_like(s0), np.zeros((3, 3))
    for idx in np.ndindex(*s0.shape):
        dp = np.zeros_like(s0)
        dp[idx] = h
        fd_s[idx] = -(energy(s0 + dp, w0) - energy(s0 - dp, w0)) / (2 * h)
    for idx in np.ndindex(3, 3):
        dw = np.zeros((3, 3))
        dw[idx] = h
        fd_w[idx] = -(energy(s0, w0 + dw) - energy(s0, w0 - dw)) / (2 * h)
    err_s, err_w = np.abs(g_s - fd_s).max() / np.abs(fd_s).max(), np.abs(g_w - fd_w).max() / np.abs(fd_w).max()
    print("generalised forces vs central differences: atoms %.2e, cell %.2e (relative)" % (err_s, err_w))
    assert np.abs(fd_s).max() > 1e-2 and np.abs(fd_w).max() > 1e-2
    assert err_s <= 1e-6 and err_w <= 1e-6


# 2 -------------------------------------------------------------------------------------------
def _toy_batch():
    """three toys in one batch: strained and rattled with a free cell; the same with its cell frozen; a mildly strained one with
    a free cell, which converges earlier"""
    starts = [strained_start(1, 0.05, 0.03), strained_start(1, 0.05, 0.03), strained_start(3, 0.01, 0.005)]
    pos = np.concatenate([p for p, _ in starts])
    cell = np.stack([c for _, c in starts])
    return pos, cell, np.array([0, 4, 8, 12]), np.array([1, 0, 1], np.uint8)


def _toy_eval(pos, cell, node_ptr):
    out = [toy_energy_forces(pos[a:b], cell[k]) for k, (a, b) in enumerate(zip(node_ptr[:-1], node_ptr[1:]))]
    return (np.array([o[0] for o in out]), np.concatenate([o[1] for o in out]).astype(np.float32), np.stack([o[2] for o in out]).astype(np.float32),
            np.array([o[3] for o in out]))


def test_reference_integrator_returns_every_bond_to_its_rest_length_and_freezes():
    pos, cell, node_ptr, cell_free = _toy_batch()
    cell_start = cell.copy()
    st, vel = new_cell_state(pos, cell, node_ptr, cell_free), np.zeros_like(pos)
    e0 = _toy_eval(pos, cell, node_ptr)[0]
    fmax, smax = 1e-4, 1e-6
    frozen_at, frozen = {}, {}
    for it in range(600):
        _, f, S, _ = _toy_eval(pos, cell, node_ptr)
        was = st["done"].copy()
        new_pos, new_cell, vel, st, diag = fire_cell_reference(pos, cell, vel, f, S, node_ptr, st, fmax, smax)
        for b in range(3):
            sl = slice(node_ptr[b], node_ptr[b + 1])
            if st["done"][b] and not was[b]:
                frozen_at[b], frozen[b] = it, (pos[sl].copy(), cell[b].copy())
                assert diag[b]["force_ok"] and diag[b]["stress_ok"] and diag[b]["fm"] < fmax              # both criteria latched
                assert cell_free[b] == 0 or diag[b]["sm"] < smax
            if st["done"][b]:                                  # to the bit, while the others go on
                assert np.array_equal(new_pos[sl], frozen[b][0]) and np.array_equal(new_cell[b], frozen[b][1]), (it, b)
        pos, cell = new_pos, new_cell
        if st["done"].all():
            break
    assert (st["done"] == 1).all(), st["done"]
    assert len(set(frozen_at.values())) == 3 and frozen_at[2] < frozen_at[0], frozen_at
    assert [int(s) for s in st["steps"]] == [frozen_at[b] for b in range(3)]
    e1, _, _, stretch = _toy_eval(pos, cell, node_ptr)
    print("toy: energies", e0, "->", e1, "largest bond error", stretch, "frozen at", frozen_at)
    assert (e1[[0, 2]] < 1e-2 * e0[[0, 2]]).all() and (stretch[[0, 2]] < 1e-3).all()                 # free cells: every bond at rest
    assert np.array_equal(cell[1], cell_start[1]) and np.array_equal(st["deform"][1], EYE)        # the frozen cell never moved
    assert e1[1] < e0[1] and stretch[1] > 1e-2                # its atoms relaxed, but a strained cell keeps strained bonds
    assert np.abs(cell[0] - cell_start[0]).max() > 0.05
    for b in (0, 2):                                          # the coordinates stayed consistent: pos = F s, C = C0 F^T
        sl = slice(node_ptr[b], node_ptr[b + 1])
        assert np.allclose(pos[sl], st["scaled"][sl] @ st["deform"][b].T, rtol=0, atol=1e-13)
        assert np.allclose(cell[b], st["cell0"][b] @ st["deform"][b].T, rtol=0, atol=1e-13)


# 3 -------------------------------------------------------------------------------------------
def frozen_inputs():
    """test_gpu_relax._fire_inputs with cells that never move: what fire_cell_step must treat exactly as fire_step does"""
    import test_gpu_relax as tgr
    pos, vel, force, node_ptr, st, fmax, fixed = tgr._fire_inputs()
    B = len(node_ptr) - 1
    rng = np.random.default_rng(5)
    cell = np.tile(EYE * 9.0, (B, 1, 1)) + 0.3 * rng.normal(size=(B, 3, 3))
    strain = rng.normal(size=(B, 3, 3)).astype(np.float32)
    cst = new_cell_state(pos, cell, node_ptr, cell_free=np.zeros(B))
    cst.update({k: st[k].copy() for k in st})
    return pos, cell, vel, force, strain, node_ptr, st, cst, fmax, fixed


def test_frozen_cells_are_the_existing_reference_to_the_bit():
    pos, cell, vel, force, strain, node_ptr, st, cst, fmax, fixed = frozen_inputs()
    rpos, rvel, rst, rdiag = trh.fire_reference(pos, vel, force, node_ptr, st, fmax, fixed)
    cpos, ccell, cvel, got, cdiag = fire_cell_reference(pos, cell, vel, force, strain, node_ptr, cst, fmax, 0.0, fixed)
    assert np.array_equal(cpos, rpos) and np.array_equal(cvel, rvel) and np.array_equal(ccell, cell)
    for k in rst:
        assert np.array_equal(got[k], rst[k]), k
    assert np.array_equal(got["deform"], cst["deform"]) and np.array_equal(got["scaled"], cpos)
    moved = [b for b in range(len(rdiag)) if rdiag[b]["branch"] != "converged"]
    assert len(moved) >= 5 and all(cdiag[b]["branch"] == rdiag[b]["branch"] for b in moved)


# 4 -------------------------------------------------------------------------------------------
def test_trust_region_stops_a_structure_at_its_last_accepted_geometry():
    """a constant tensile strain gradient drives the cell of one toy outwards; the step that would cross |F - I| = max_deform is
    not made, the structure is latched with status 2 and later calls leave it alone.  A second toy in the batch is not affected."""
    starts = [strained_start(1, 0.0, 0.0), strained_start(3, 0.01, 0.005)]
    pos, cell, node_ptr = np.concatenate([p for p, _ in starts]), np.stack([c for _, c in starts]), np.array([0, 4, 8])
    st, vel = new_cell_state(pos, cell, node_ptr, cell_factor=[1.0, 4.0]), np.zeros_like(pos)
    f = np.zeros((8, 3), np.float32)
    S = np.stack([-1.0 * EYE, 1e-3 * EYE]).astype(np.float32)
    last, stopped_at = None, None
    for it in range(40):
        new = fire_cell_reference(pos, cell, vel, f, S, node_ptr, st, 0.0, 0.0, max_deform=0.2)
        d = new[4][0]
        if stopped_at is None and new[3]["done"][0] == 2:
            stopped_at, last = it, (pos[:4].copy(), cell[0].copy(), st["deform"][0].copy(), vel[:4].copy(), int(st["steps"][0]))
            assert d["branch"] == "stopped" and d["dev"] > 0.2 * (1 + 1e-3)
        elif stopped_at is None:
            assert d["dev"] < 0.2 * (1 - 1e-3), d                                # no marginal decision
        pos, cell, vel, st = new[:4]
        if stopped_at is not None:
            assert st["done"][0] == 2 and new[4][0]["branch"] in ("stopped", "latched")
            assert np.array_equal(pos[:4], last[0]) and np.array_equal(cell[0], last[1]) and np.array_equal(st["deform"][0], last[2])
            assert np.array_equal(vel[:4], last[3]) and int(st["steps"][0]) == last[4]
    assert stopped_at is not None and stopped_at > 1
    dev = np.sqrt(((st["deform"][0] - EYE) ** 2).sum())
    assert 0.1 < dev <= 0.2 and det3(cell[0]) > det3(starts[0][1])               # it did expand, and stopped inside the region
    assert st["done"][1] == 0 and st["steps"][1] == 40                           # the neighbour went on


# ---------------------------------------------------------------------------------------------
# 5. the oracle CGCNN at held lists: the reference trajectory of tests/test_gpu_relax_cell.py
# ---------------------------------------------------------------------------------------------
RELAX_CELL_ARGS = dict(steps=20, dt=3.0, dt_max=30.0, fmax=0.0, smax=0.0, cell_factor=None)


def oracle_energy_forces_strain(case, pos, cell):
    """per-structure energies, F = -dE/dpos and S = dE/d eps (autograd w.r.t. a zero strain of positions and image shifts, fp64) of
    the oracle on the HELD lists; the minimum image of every edge is chosen anew from `pos` and `cell`"""
    import types
    from oracle import ops as oops
    p = case.p
    sh = torch.from_numpy(edge_shifts(pos, p["node_ptr"], cell, p["pbc"], case.src, case.tgt))
    s, t = torch.from_numpy(case.src), torch.from_numpy(case.tgt)
    B = len(p["node_ptr"]) - 1
    pg_ = torch.from_numpy(np.asarray(pos, np.float64)).requires_grad_(True)
    eps = torch.zeros(B, 3, 3, dtype=torch.float64, requires_grad=True)
    d = edge_dist(*tsh.strained(pg_, sh, eps, case.batch, case.batch[s]), s, t)
    lo, hi = tgf.DIST_RANGE
    data = types.SimpleNamespace(x=case.x, edge_index=torch.stack([s, t]), edge_attr=oops.rbf_expand((d - lo) / (hi - lo)), batch=case.batch,
                                 num_graphs=B)
    pred = case.model(data)
    g, ge = torch.autograd.grad(pred.sum(), [pg_, eps])
    return pred.detach().numpy().copy(), -g.numpy(), ge.numpy()


def reference_cell_trajectory(case, steps, dt, dt_max, fmax, smax, cell_factor, noise=0.0, seed=0):
    """positions, cells, energies and diagnostics of `steps` updates in fp64; noise: every force component perturbed by uniform
    noise of amplitude noise * max|F| and every component of S by noise * max|S| before the integrator sees them"""
    rng = np.random.default_rng(seed)
    node_ptr = case.p["node_ptr"]
    pos, cell, vel = case.p["pos"].copy(), case.p["cell"].copy(), np.zeros_like(case.p["pos"])
    st = new_cell_state(pos, cell, node_ptr, cell_factor=cell_factor, dt=dt)
    energies, diags = [], []
    for _ in range(steps):
        e, f, S = oracle_energy_forces_strain(case, pos, cell)
        if noise:
            f = f + rng.uniform(-1.0, 1.0, f.shape) * noise * np.abs(f).max()
            S = S + rng.uniform(-1.0, 1.0, S.shape) * noise * np.abs(S).max()
        pos, cell, vel, st, dg = fire_cell_reference(pos, cell, vel, f, S, node_ptr, st, fmax, smax, dt_max=dt_max)
        energies.append(e)
        diags.append(dg)
    energies.append(oracle_energy_forces_strain(case, pos, cell)[0])
    return pos, cell, np.asarray(energies), diags, st


@functools.lru_cache(maxsize=None)
def cgcnn_cell_reference():
    return reference_cell_trajectory(trh.cgcnn_case(), **RELAX_CELL_ARGS)


def test_oracle_cgcnn_goes_downhill_with_its_cell_and_noise_sensitivity():
    """20 steps with dt = 3, dt_max = 30, fmax = smax = 0 and the default cell_factor (the number of atoms) on the structures of
    test_relax_host.cgcnn_case.  Measured here: every energy drops (by 1.9e-3 to 7.5e-3 from 6.2e-3 to
    2.0e-2), no downhill reset, atoms travel up to 1.70 A, lattice vectors move by 0.07 to 0.88 A, |F - I| stays below 0.26,
    DEV_POS = 1.49e-4 A, DEV_CELL = 3.42e-5 A."""
    case = trh.cgcnn_case()
    pos, cell, energies, diags, st = cgcnn_cell_reference()
    B = len(case.p["node_ptr"]) - 1
    e0, f0, s0 = oracle_energy_forces_strain(case, case.p["pos"], case.p["cell"])
    assert np.array_equal(f0, trh.oracle_energy_forces(case, case.p["pos"])[1])               # the forces of the fixed-cell oracle
    assert np.abs(s0 - s0.transpose(0, 2, 1)).max() <= 1e-12 * np.abs(s0).max()
    assert (st["steps"] == RELAX_CELL_ARGS["steps"]).all() and not st["done"].any() and st["cell_free"].all()
    drop = energies[0] - energies[-1]
    moved = np.sqrt(((pos - case.p["pos"]) ** 2).sum(1)).max()
    cell_moved = np.sqrt(((cell - case.p["cell"]) ** 2).sum(2)).max(1)
    print("energies at the start", energies[0], "drops", drop, "largest displacement %.3e A" % moved, "lattice vectors moved", cell_moved)
    assert (drop > 0).all(), drop
    assert (cell_moved > 0.02).all(), cell_moved                                               # visibly: hundreds of times the bound
    assert max(dg[b]["dev"] for dg in diags for b in range(B)) < 0.4                           # inside the trust region (0.5) with a margin
    for it, dg in enumerate(diags):
        for b in range(B):
            if it == 0:
                assert dg[b]["branch"] == "first"
            else:                                             # P > 0 with a margin: no branch of the trajectory depends on rounding
                assert dg[b]["branch"] in ("uphill-free", "accelerate") and dg[b]["P"] >= 1e-3 * dg[b]["abs_fv"], (it, b, dg[b])
    noisy = reference_cell_trajectory(case, noise=1e-4, seed=1, **RELAX_CELL_ARGS)
    dev_pos = float(np.sqrt(((noisy[0] - pos) ** 2).sum(1)).max())
    dev_cell = float(np.sqrt(((noisy[1] - cell) ** 2).sum(2)).max())
    print("DEV_POS = %.3e A (TRAJ_BOUND_POS %.1e), DEV_CELL = %.3e A (TRAJ_BOUND_CELL %.1e)" % (dev_pos, TRAJ_BOUND_POS, dev_cell, TRAJ_BOUND_CELL))
    assert 0.0 < dev_pos <= TRAJ_BOUND_POS / 10 and 0.0 < dev_cell <= TRAJ_BOUND_CELL / 10


# ---------------------------------------------------------------------------------------------
# 6. surface
# ---------------------------------------------------------------------------------------------
def test_cell_relaxation_surface_exists_and_relax_is_what_it_was():
    from matdeeplearn_amd import _build, _lib, forces, ops
    assert callable(forces.relax_cell) and callable(forces.ForceField.set_cell) and callable(ops.fire_cell_step) and callable(ops.fire_cell_state)
    assert ops.FIRE_CELL_CONSTANTS == FIRE_CELL_CONSTANTS and ops.FIRE_CONSTANTS == trh.FIRE_CONSTANTS
    assert forces.CellRelaxResult._fields == ("positions", "cell", "energy", "forces", "stress", "converged", "steps", "fmax", "smax", "status",
                                              "node_ptr")
    assert ops.FireCellState.__slots__[:6] == ops.FireState.__slots__
    pos, cell, ptr = torch.zeros(2, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64).unsqueeze(0), torch.tensor([0, 2])
    with pytest.raises(ops.MdlError, match="HIP device"):
        ops.fire_cell_state(pos, cell, ptr)
    with pytest.raises(ops.MdlError, match="HIP device"):
        ops.fire_cell_step(pos, cell, pos.clone(), torch.zeros(2, 3), torch.zeros(1, 3, 3), ptr, ops.FireCellState(*[torch.zeros(1)] * 13), 0.05,
                           1e-3)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mdl_hip.h")).read()
    assert "mdl_fire_cell_step" in _lib.PROTOTYPES and re.search(r"\bmdl_fire_cell_step\(", header)
    if os.path.exists(_build.LIB):
        assert hasattr(_lib.lib(), "mdl_fire_cell_step")
    assert str(inspect.signature(forces.relax)) == (
        "(model, structs, dist_range, fmax=0.05, steps=200, rebuild_every=1, fixed=None, dt=0.1, dt_max=1.0, maxstep=0.2, n_min=5, "
        "f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, check_every=10, radius=8.0, max_neighbors=12, dictionary=None, output_index=None)")
    assert forces.RelaxResult._fields == ("positions", "energy", "forces", "converged", "steps", "fmax", "node_ptr")
    sig = inspect.signature(forces.relax_cell)
    assert list(sig.parameters)[:11] == ["model", "structs", "dist_range", "fmax", "smax", "steps", "rebuild_every", "fixed", "cell_free",
                                         "cell_factor", "max_deform"]
    assert sig.parameters["max_deform"].default == 0.5 and sig.parameters["rebuild_every"].default == 1


def test_both_fire_steps_check_their_arguments_under_their_own_name():
    """One checker serves ops.fire_step and ops.fire_cell_step; what it finds before it asks for a device is reported with the name of
    the function that was called (a state field of the wrong dtype is found behind that: tests/test_gpu_relax_cell.py)."""
    from matdeeplearn_amd import ops
    pos, cell, ptr = torch.zeros(2, 3, dtype=torch.float64), torch.eye(3, dtype=torch.float64).unsqueeze(0), torch.tensor([0, 2])
    state, cell_state = ops.FireState(*[torch.zeros(1)] * 6), ops.FireCellState(*[torch.zeros(1)] * 13)
    step = lambda st, **kw: ops.fire_step(pos, pos.clone(), torch.zeros(2, 3), ptr, st, 0.05, **kw)
    cell_step = lambda st, **kw: ops.fire_cell_step(pos, cell, pos.clone(), torch.zeros(2, 3), torch.zeros(1, 3, 3), ptr, st, 0.05, 1e-3, **kw)
    with pytest.raises(ops.MdlError, match=r"^fire_step: unknown constants \['max_deform'\]"):     # the cell's constant is none of fire_step's
        step(state, max_deform=0.2)
    with pytest.raises(ops.MdlError, match=r"^fire_cell_step: unknown constants \['max_step'\]"):
        cell_step(cell_state, max_deform=0.2, max_step=0.1)
    with pytest.raises(ops.MdlError, match=r"^fire_step: state must be an ops\.FireState \(ops\.fire_state\)"):
        step(cell_state)
    with pytest.raises(ops.MdlError, match=r"^fire_cell_step: state must be an ops\.FireCellState \(ops\.fire_cell_state\)"):
        cell_step(state)
