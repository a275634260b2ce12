"""Host side of the relaxation tests: this file OWNS the reference of the batched FIRE update (csrc/relax.hip, ops.fire_step,
forces.relax) — fire_reference, a numpy fp64 restatement of the update as include/mdl_hip.h states it, one structure after the
other — and the fp64 reference trajectory of the oracle CGCNN at held neighbour lists that tests/test_gpu_relax.py compares
forces.relax with.  The upstream reference moves no atoms, so no golden from it exists.  No GPU.

TRAJ_BOUND, the bound of that comparison, is the reference's own sensitivity: the same 20 steps with every force perturbed by
uniform noise of amplitude 1e-4 max|F| (the bound tests/test_gpu_forces._check_forces puts on the device forces) moved the final
positions by DEV = 1.45e-4 A at most (measured here; the atoms travel up to 1.41 A); TRAJ_BOUND = 10 x DEV, rounded up to two
digits, by the project's "measured x 10" rule."""
import functools
import types

import numpy as np
import pytest
import torch

import test_gpu_forces as tgf
from oracle import models as omodels
from oracle import ops as oops
from test_forces_host import edge_dist, edge_shifts

TRAJ_BOUND = 1.5e-3           # A; 10 x the DEV measured below (see the module docstring)
FIRE_CONSTANTS = dict(n_min=5, f_inc=1.1, f_dec=0.5, alpha_start=0.1, f_alpha=0.99, dt_max=1.0, maxstep=0.2)


def new_state(B, dt=0.1, alpha=0.1):
    return {"dt": np.full(B, dt), "alpha": np.full(B, alpha), "n_pos": np.zeros(B, np.int32), "steps": np.zeros(B, np.int32),
            "done": np.zeros(B, np.int32), "fmax_seen": np.zeros(B, np.float32)}


def fire_reference(pos, vel, force, node_ptr, state, fmax, fixed=None, **constants):
    """One FIRE update of every structure, fp64.  Returns (pos, vel, state, diag) as NEW arrays; diag[b] holds the numbers the
    decisions of structure b were taken from (fm, P, sum |f.v|, s, branch) so a test can tell whether one of them was marginal."""
    c = dict(FIRE_CONSTANTS, **constants)
    pos, vel = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
    force = np.asarray(force, dtype=np.float64)
    st = {k: np.array(v) for k, v in state.items()}
    B = len(node_ptr) - 1
    fmax = np.broadcast_to(np.asarray(fmax, dtype=np.float64), (B,))
    free_all = np.ones(len(pos), bool) if fixed is None else ~np.asarray(fixed).astype(bool)
    diag = []
    for b in range(B):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        free = free_all[a:e]
        f = np.where(free[:, None], force[a:e], 0.0)
        v = np.where(free[:, None], vel[a:e], 0.0)
        fm = float(np.sqrt((f * f).sum(1)).max()) if e > a else 0.0
        st["fmax_seen"][b] = np.float32(fm)
        d = {"fm": fm, "P": 0.0, "abs_fv": 0.0, "s": 0.0, "branch": "converged"}
        diag.append(d)
        if st["done"][b] != 0 or fm < fmax[b] or fm == 0.0:
            st["done"][b] = 1
            continue
        dt, alpha = float(st["dt"][b]), float(st["alpha"][b])
        if st["steps"][b] == 0:
            d["branch"] = "first"
        else:
            P = float((f * v).sum())
            d["P"], d["abs_fv"] = P, float(np.abs((f * v).sum(1)).sum())
            if P > 0.0:
                v = (1.0 - alpha) * v + alpha * (np.sqrt((v * v).sum()) / np.sqrt((f * f).sum())) * f
                d["branch"] = "uphill-free"
                if st["n_pos"][b] > c["n_min"]:
                    dt = min(dt * c["f_inc"], c["dt_max"])
                    alpha = alpha * c["f_alpha"]
                    d["branch"] = "accelerate"
                st["n_pos"][b] += 1
            else:
                v = np.zeros_like(v)
                alpha, dt = c["alpha_start"], dt * c["f_dec"]
                st["n_pos"][b] = 0
                d["branch"] = "reset"
        v = v + dt * f
        dr = dt * v
        s = float(np.sqrt((dr * dr).sum()))
        d["s"] = s
        if s > c["maxstep"]:
            dr = dr * (c["maxstep"] / s)
        pos[a:e] += dr
        vel[a:e] = v
        st["dt"][b], st["alpha"][b] = dt, alpha
        st["steps"][b] += 1
    return pos, vel, st, diag


# ---------------------------------------------------------------------------------------------
# 1. quadratic bowls
# ---------------------------------------------------------------------------------------------
def test_quadratic_bowls_converge_one_after_the_other_and_stay_frozen():
    from matdeeplearn_amd import forces, ops
    assert callable(forces.relax) and callable(forces.ForceField)
    assert ops.FIRE_CONSTANTS == FIRE_CONSTANTS                 # the restatement and the product start from the same constants
    with pytest.raises(ops.MdlError, match="HIP device"):       # and the product has no CPU path
        ops.fire_step(torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3, dtype=torch.float64), torch.zeros(2, 3),
                      torch.tensor([0, 2]), ops.FireState(*[torch.zeros(1)] * 6), 0.05)
    rng = np.random.default_rng(0)
    sizes, stiff = [5, 9, 3], np.array([1.0, 10.0, 100.0])
    node_ptr = np.concatenate([[0], np.cumsum(sizes)])
    k = np.repeat(stiff, sizes)[:, None]
    x0 = rng.normal(size=(sum(sizes), 3))
    pos = x0 + 0.3 * rng.normal(size=x0.shape)
    vel, st = np.zeros_like(pos), new_state(3)
    frozen_at, frozen_pos = {}, {}
    e0 = [float((0.5 * k * (pos - x0) ** 2)[node_ptr[b]:node_ptr[b + 1]].sum()) for b in range(3)]
    for it in range(400):
        f = (-k * (pos - x0)).astype(np.float32)
        was = st["done"].copy()
        new_pos, vel, st, _ = fire_reference(pos, vel, f, node_ptr, st, 0.05)
        for b in range(3):
            sl = slice(node_ptr[b], node_ptr[b + 1])
            if st["done"][b] and not was[b]:
                frozen_at[b], frozen_pos[b] = it, pos[sl].copy()
            if st["done"][b]:
                assert np.array_equal(new_pos[sl], frozen_pos[b]), (it, b)          # to the bit, while the others go on
                assert np.sqrt(((-k * (new_pos - x0))[sl] ** 2).sum(1)).max() < 0.05
        pos = new_pos
        if st["done"].all():
            break
    assert st["done"].all(), st
    assert len(set(frozen_at.values())) == 3, frozen_at                          # three different step counts
    assert [int(s) for s in st["steps"]] == [frozen_at[b] for b in range(3)]      # steps counts updates made, not calls
    e1 = [float((0.5 * k * (pos - x0) ** 2)[node_ptr[b]:node_ptr[b + 1]].sum()) for b in range(3)]
    assert all(b < 1e-2 * a for a, b in zip(e0, e1)), (e0, e1)


# ---------------------------------------------------------------------------------------------
# 2. the oracle CGCNN at held lists: the reference trajectory of tests/test_gpu_relax.py
# ---------------------------------------------------------------------------------------------
RELAX_ARGS = dict(steps=20, dt=3.0, dt_max=30.0, fmax=0.0)


@functools.lru_cache(maxsize=None)
def cgcnn_case():
    """structures, host-built graphs (held throughout) and the fp64 oracle CGCNN of the trajectory comparison"""
    from matdeeplearn_amd.process import graph as pg
    structs = tgf._bulk_structures(6, seed=0, lo=4, hi=20)
    p = tgf._pack(structs)
    xs, src, tgt = [], [], []
    for b, s in enumerate(structs):
        g = pg.build_graph(s["positions"], s["numbers"], s["cell"], s["pbc"])
        ei = pg.sort_by_target(g["edge_index"])[0] + p["node_ptr"][b]
        xs.append(g["x"])
        src.append(ei[0])
        tgt.append(ei[1])
    torch.manual_seed(0)
    model = omodels.CGCNN(tgf.DS(), dim1=64, dim2=64, gc_count=2, post_fc_count=1)
    with torch.no_grad():
        for bn in model.bn_list:
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
    state_dict = {k: v.clone() for k, v in model.state_dict().items()}
    model = model.double().eval()
    batch = torch.from_numpy(np.repeat(np.arange(len(structs)), np.diff(p["node_ptr"])))
    return types.SimpleNamespace(structs=structs, p=p, x=torch.from_numpy(np.concatenate(xs)).double(), src=np.concatenate(src),
                                 tgt=np.concatenate(tgt), batch=batch, model=model, state_dict=state_dict)


def oracle_energy_forces(case, pos):
    """per-structure energies and F = -dE/dpos of the fp64 oracle on the HELD lists; the minimum image of every edge is chosen
    anew from `pos` (as the device geometry does), then held under the derivative"""
    p = case.p
    sh = torch.from_numpy(edge_shifts(pos, p["node_ptr"], p["cell"], p["pbc"], case.src, case.tgt))
    s, t = torch.from_numpy(case.src), torch.from_numpy(case.tgt)
    pg_ = torch.from_numpy(np.asarray(pos, np.float64)).requires_grad_(True)
    d = edge_dist(pg_, sh, s, t)
    lo, hi = tgf.DIST_RANGE
    data = types.SimpleNamespace(x=case.x, edge_index=torch.stack([s, t]), edge_attr=oops.rbf_expand((d - lo) / (hi - lo)), batch=case.batch,
                                 num_graphs=len(p["node_ptr"]) - 1)
    pred = case.model(data)
    (g,) = torch.autograd.grad(pred.sum(), pg_)
    return pred.detach().numpy().copy(), -g.numpy()


def reference_trajectory(case, steps, dt, dt_max, fmax, noise=0.0, seed=0):
    """positions, energies and diagnostics of `steps` FIRE updates in fp64; noise: every force component perturbed by uniform
    noise of amplitude noise * max|F| before the integrator sees it"""
    rng = np.random.default_rng(seed)
    node_ptr = case.p["node_ptr"]
    pos, vel, st = case.p["pos"].copy(), np.zeros_like(case.p["pos"]), new_state(len(node_ptr) - 1, dt=dt)
    energies, diags = [], []
    for _ in range(steps):
        e, f = oracle_energy_forces(case, pos)
        if noise:
            f = f + rng.uniform(-1.0, 1.0, f.shape) * noise * np.abs(f).max()
        pos, vel, st, dg = fire_reference(pos, vel, f, node_ptr, st, fmax, dt_max=dt_max)
        energies.append(e)
        diags.append(dg)
    energies.append(oracle_energy_forces(case, pos)[0])
    return pos, np.asarray(energies), diags, st


@functools.lru_cache(maxsize=None)
def cgcnn_reference():
    return reference_trajectory(cgcnn_case(), **RELAX_ARGS)


def test_oracle_cgcnn_goes_downhill_at_held_lists_and_noise_sensitivity():
    """20 steps with dt = 3, dt_max = 30, fmax = 0 (an untrained model's forces are of order 1e-3 per A).  Measured here: energy
    drops of 1.9e-3 to 7.1e-3 per structure from energies of 6.2e-3 to 2.0e-2, no downhill reset, largest displacement of an atom
    1.41 A, DEV = 1.45e-4 A."""
    case = cgcnn_case()
    pos, energies, diags, st = cgcnn_reference()
    B = len(case.p["node_ptr"]) - 1
    assert (st["steps"] == RELAX_ARGS["steps"]).all() and not st["done"].any()
    drop = energies[0] - energies[-1]
    moved = np.sqrt(((pos - case.p["pos"]) ** 2).sum(1)).max()
    print("energies at the start", energies[0], "drops", drop, "largest displacement %.3e A" % moved)
    assert (drop > 0).all(), drop
    for it, dg in enumerate(diags):
        for b in range(B):
            if it == 0:
                assert dg[b]["branch"] == "first"
            else:                                             # P > 0 with a margin: no branch of the trajectory depends on rounding
                assert dg[b]["branch"] in ("uphill-free", "accelerate") and dg[b]["P"] >= 1e-3 * dg[b]["abs_fv"], (it, b, dg[b])
    noisy = reference_trajectory(case, noise=1e-4, seed=1, **RELAX_ARGS)[0]
    dev = float(np.sqrt(((noisy - pos) ** 2).sum(1)).max())
    print("DEV = %.3e A (TRAJ_BOUND %.1e)" % (dev, TRAJ_BOUND))
    assert 0.0 < dev <= TRAJ_BOUND / 10
