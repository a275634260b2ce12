#!/usr/bin/env python3
"""Relaxation step on the device: what one step of forces.relax costs, phase by phase, and the integrator against the same update
composed from torch ops.

  python tools/bench_relax.py [--model cgcnn|schnet] [--graphs 64,1024] [--dim 64] [--steps 20] [--repeats 5] [--seed 0] [--cell]

Structures as tools/bench_forces.py draws them (n ~ lognormal(ln 20, 0.7) clipped to [1, 200], cubic periodic cell at density
0.05); a seeded model in eval mode, fp32.  One JSON line per batch size:
  rebuild_ms / evaluate_ms / fire_ms   device events around ForceField.rebuild(), ForceField.evaluate() and ops.fire_step of every
                                       step of a --steps long relaxation (dt = 3, fmax = 0: every structure moves in every step),
                                       mean per step, best of --repeats runs
  call_ms           one forces.energy_and_forces call on the same structures (host packing and upload included): what a step cost
                    before ForceField, to set against rebuild_ms + evaluate_ms
  fire_us / torch_us   the integrator alone on the forces of the first step, the HIP launch against torch_fire_step below (the
                    same update from elementwise ops and index_add_ / scatter_reduce_ over the structures), taking turns, best of
                    repeats, on clones of one state
  max_pos_diff      largest difference between the positions the two produce in that one step
  fire_repeatable / torch_repeatable   whether 5 runs from the same inputs gave the same bits
--cell: the step of forces.relax_cell instead — evaluate_ms is ForceField.evaluate(stress=True, volume_normalised=False), fire_ms is
ops.fire_cell_step with every cell free, and the integrator-alone part adds fire_cell_us / fire_cell_repeatable (ops.fire_cell_step
on the same forces and the strain gradient of the first step, taking turns with the other two)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_forces import DS, structures  # noqa: E402
from matdeeplearn_amd import forces, models, ops  # noqa: E402
from matdeeplearn_amd.process import graph as pg  # noqa: E402


def torch_fire_step(pos, vel, force, batch, st, fmax, fixed, c):
    """ops.fire_step from torch ops, in place, no host decision: four segmented sums and a segmented max between elementwise passes"""
    B = st.dt.numel()
    free = None if fixed is None else (fixed == 0).unsqueeze(1)
    f = force.double() if free is None else force.double() * free
    v = vel if free is None else vel * free
    seg = lambda x: torch.zeros(B, dtype=torch.float64, device=pos.device).index_add_(0, batch, x)
    f2 = (f * f).sum(1)
    fm = torch.zeros(B, dtype=torch.float64, device=pos.device).scatter_reduce_(0, batch, f2, "amax").sqrt()
    move = ~((st.done != 0) | (fm < fmax) | (fm == 0))
    P, vv, ff = seg((f * v).sum(1)), seg((v * v).sum(1)), seg(f2)
    first = st.steps == 0
    mix, reset = ~first & (P > 0), ~first & ~(P > 0)
    grow = mix & (st.n_pos > c["n_min"])
    one, zero = torch.ones_like(st.dt), torch.zeros_like(st.dt)
    c_v = torch.where(first, one, torch.where(mix, 1.0 - st.alpha, zero))
    c_f = torch.where(mix, st.alpha * (vv.sqrt() / torch.where(ff > 0, ff, one).sqrt()), zero)
    dt = torch.where(grow, (st.dt * c["f_inc"]).clamp(max=c["dt_max"]), torch.where(reset, st.dt * c["f_dec"], st.dt))
    alpha = torch.where(grow, st.alpha * c["f_alpha"], torch.where(reset, torch.full_like(st.alpha, c["alpha_start"]), st.alpha))
    n_pos = torch.where(mix, st.n_pos + 1, torch.where(reset, torch.zeros_like(st.n_pos), st.n_pos))
    dtb = dt[batch].unsqueeze(1)
    vn = (c_v[batch].unsqueeze(1) * v + c_f[batch].unsqueeze(1) * f) + dtb * f
    dr = dtb * vn
    s = seg((dr * dr).sum(1)).sqrt()
    clip = torch.where(s > c["maxstep"], c["maxstep"] / torch.where(s > 0, s, one), one)
    mb = move[batch].unsqueeze(1)
    pos.add_(torch.where(mb, dr * clip[batch].unsqueeze(1), torch.zeros_like(dr)))
    vel.copy_(torch.where(mb, vn, vel))
    st.dt.copy_(torch.where(move, dt, st.dt))
    st.alpha.copy_(torch.where(move, alpha, st.alpha))
    st.n_pos.copy_(torch.where(move, n_pos, st.n_pos))
    st.steps.add_(move.to(torch.int32))
    st.done.copy_((~move).to(torch.int32))
    st.fmax_seen.copy_(fm.float())
    return st


def events(n):
    return [torch.cuda.Event(enable_timing=True) for _ in range(n)]


def make_model(a, dev):
    torch.manual_seed(a.seed)
    if a.model == "schnet":
        return models.SchNet(DS(), dim1=a.dim, dim2=a.dim, dim3=a.dim, gc_count=3, post_fc_count=1).to(dev).eval()
    return models.CGCNN(DS(), dim1=a.dim, dim2=a.dim, gc_count=4, post_fc_count=1).to(dev).eval()


def relaxation_phases(model, packed, steps, const, cell=False):
    """one relaxation, every step rebuilt: per-step means (ms) of the three phases"""
    ff = forces.ForceField(model, packed, (0.0, 8.0))
    B = ff.node_ptr.numel() - 1
    if cell:
        state = ops.fire_cell_state(ff.positions, ff.cell, ff.node_ptr, dt=3.0)
    else:
        state = ops.fire_state(B, 3.0, 0.1, ff.positions.device)
    vel = torch.zeros_like(ff.positions)
    fmax = torch.zeros(B, dtype=torch.float64, device=ff.positions.device)
    marks = []
    for _ in range(steps):
        e = events(4)
        e[0].record()
        ff.rebuild()
        e[1].record()
        if cell:
            _, f, strain = ff.evaluate(stress=True, volume_normalised=False)
            e[2].record()
            ops.fire_cell_step(ff.positions, ff.cell, vel, f, strain, ff.node_ptr, state, fmax, fmax, **const)
        else:
            _, f = ff.evaluate()
            e[2].record()
            ops.fire_step(ff.positions, vel, f, ff.node_ptr, state, fmax, **const)
        e[3].record()
        marks.append(e)
    torch.cuda.synchronize()
    return [sum(e[k].elapsed_time(e[k + 1]) for e in marks) / steps for k in range(3)]


def integrator_alone(model, packed, repeats, const, cell=False):
    ff = forces.ForceField(model, packed, (0.0, 8.0))
    dev, B, N = ff.positions.device, ff.node_ptr.numel() - 1, ff.positions.shape[0]
    if cell:
        _, f, strain = ff.evaluate(stress=True, volume_normalised=False)
    else:
        _, f = ff.evaluate()
    batch = torch.repeat_interleave(torch.arange(B, device=dev), ff.node_ptr[1:] - ff.node_ptr[:-1], output_size=N)
    state0 = ops.fire_state(B, 3.0, 0.1, dev)
    state0.steps.fill_(3)                                       # past the first step: the mixing branch runs
    state0.n_pos.fill_(7)
    vel0 = 0.5 * f.double()
    fmax = torch.zeros(B, dtype=torch.float64, device=dev)
    c = dict(ops.FIRE_CONSTANTS, **const)

    def hip():
        pos, vel, st = ff.positions.clone(), vel0.clone(), state0.clone()
        e = events(2)
        e[0].record()
        ops.fire_step(pos, vel, f, ff.node_ptr, st, fmax, **const)
        e[1].record()
        return e, pos

    def composed():
        pos, vel, st = ff.positions.clone(), vel0.clone(), state0.clone()
        e = events(2)
        e[0].record()
        torch_fire_step(pos, vel, f, batch, st, fmax, None, c)
        e[1].record()
        return e, pos

    if cell:
        cstate0 = ops.fire_cell_state(ff.positions, ff.cell, ff.node_ptr, dt=3.0)
        cstate0.steps.fill_(3)
        cstate0.n_pos.fill_(7)
        cstate0.vel_cell.copy_(-0.5 * strain.double() / cstate0.cell_factor.view(-1, 1, 1))   # along the cell's force at F = I

    def hip_cell():
        pos, cl, vel, st = ff.positions.clone(), ff.cell.clone(), vel0.clone(), cstate0.clone()
        e = events(2)
        e[0].record()
        ops.fire_cell_step(pos, cl, vel, f, strain, ff.node_ptr, st, fmax, fmax, **const)
        e[1].record()
        return e, pos

    fns = (hip, composed, hip_cell) if cell else (hip, composed)
    for fn in fns:
        fn()
    best, outs = [None] * len(fns), [[] for _ in fns]
    for _ in range(max(repeats, 5)):
        for k, fn in enumerate(fns):
            e, pos = fn()
            torch.cuda.synchronize()
            t = e[0].elapsed_time(e[1])
            best[k] = t if best[k] is None else min(best[k], t)
            outs[k].append(pos)
    same = lambda ps: all(torch.equal(ps[0], p) for p in ps[1:5])
    out = {"fire_us": round(best[0] * 1e3, 1), "torch_us": round(best[1] * 1e3, 1),
           "max_pos_diff": float((outs[0][0] - outs[1][0]).abs().max()), "fire_repeatable": same(outs[0]), "torch_repeatable": same(outs[1])}
    if cell:
        out.update({"fire_cell_us": round(best[2] * 1e3, 1), "fire_cell_repeatable": same(outs[2])})
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("cgcnn", "schnet"), default="cgcnn")
    ap.add_argument("--graphs", default="64,1024")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--cell", action="store_true", help="time the step of forces.relax_cell (stress and ops.fire_cell_step)")
    a = ap.parse_args()
    dev = torch.device("cuda")
    const = dict(dt_max=30.0)
    model = make_model(a, dev)
    for B in [int(v) for v in a.graphs.split(",")]:
        packed = pg.pack_structures(structures(B, a.seed))
        relaxation_phases(model, packed, 2, const, a.cell)                 # warm-up (code objects, allocator)
        best = None
        for _ in range(a.repeats):
            t = relaxation_phases(model, packed, a.steps, const, a.cell)
            best = t if best is None else [min(x, y) for x, y in zip(best, t)]
        forces.energy_and_forces(model, packed, (0.0, 8.0))
        call = None
        for _ in range(a.repeats):
            e = events(2)
            e[0].record()
            forces.energy_and_forces(model, packed, (0.0, 8.0))
            e[1].record()
            torch.cuda.synchronize()
            t = e[0].elapsed_time(e[1])
            call = t if call is None else min(call, t)
        line = {"model": a.model, "cell": a.cell, "graphs": B, "atoms": int(packed["node_ptr"][-1]), "dim": a.dim, "steps": a.steps,
                "rebuild_ms": round(best[0], 3), "evaluate_ms": round(best[1], 3), "fire_ms": round(best[2], 4), "call_ms": round(call, 3)}
        line.update(integrator_alone(model, packed, a.repeats, const, a.cell))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
