#!/usr/bin/env python3
"""Molecular-dynamics step on the device: what one step of forces.md costs, phase by phase, and the integrator against the same
update composed from torch ops.

  python tools/bench_md.py [--model cgcnn|schnet] [--graphs 64,1024] [--dim 64] [--steps 20] [--repeats 5] [--seed 0] [--npt] [--observe] [--vacf] [--sq]

Structures and model as tools/bench_relax.py takes them; masses uniform in [1, 4], dt = 1, Langevin at gamma = 0.05, kT = 2e-5 (an
untrained model's forces are of order 1e-3 per A), Maxwell-Boltzmann velocities.  One JSON line per batch size:
  rebuild_ms / evaluate_ms / md_ms   device events around ForceField.rebuild(), ForceField.evaluate() and ops.md_step of every step
                                     of a --steps long run with rebuild_every = 1, mean per step, best of --repeats runs
  stopped           structures the guard (max_disp = 0.5) stopped in such a run: 0 unless the time step is too long for the forces
  md_us / md_nve_us / torch_us   the integrator alone on the forces of the first step: the HIP launch with and without the thermostat
                    against torch_md_step below (the Langevin update from elementwise ops, torch.randn and index_add_ over the
                    structures), taking turns, best of repeats, on clones of one state
  max_pos_diff      largest difference between the positions md_nve_us and the composition without noise produce in that one step
  md_repeatable / torch_repeatable   whether 5 runs from the same inputs gave the same bits (torch.randn draws from the process's
                    generator: the composed step repeats only if nothing else has drawn in between)
--npt adds the step of forces.md_npt from the same run (target pressure 0, rate = compressibility / tau_p = 30, max_strain = 0.03):
  npt_rebuild_ms / npt_evaluate_ms / npt_md_ms / npt_stopped   the phases above with ForceField.evaluate(stress=True,
                    volume_normalised=False) and ops.md_cell_step in the place of evaluate() and ops.md_step
  md_cell_us        ops.md_cell_step alone on the forces and the strain gradient of the first step, taking turns with the others
--observe adds what forces.sample costs when it samples EVERY step (every = 1; rdf: 256 bins to 8 A; msd: 64 lags, a new origin
every 4 samples; three types, Z mod 3 — one type per atomic number of these random structures would not fit the histogram), from a
run of its own in which the sampling calls are a fourth phase between rebuild and evaluate:
  obs_rebuild_ms / obs_evaluate_ms / obs_md_ms   the three phases above in that run: their sum, step_ms, is the un-observed step
  observe_ms        ops.rdf_accumulate + ops.msd_accumulate (and the copy of a new origin) per step, mean over the run, best of repeats
  step_ms / step_observed_ms   the sum without and with observe_ms.  The ring holds 16 origins and is full after 64 samples: use
                    --steps 80 or more for the steady state
--vacf adds what forces.sample costs when a forces.Correlate samples the velocities at EVERY step (every = 1; vacf: 64 lags, a new
origin every 4 samples; three types), from a run of its own in which the velocity calls are a fourth phase between evaluate and md:
  vacf_rebuild_ms / vacf_evaluate_ms / vacf_md_ms   the three phases above in that run: their sum, vacf_step_ms, is the un-sampled step
  vacf_ms           ops.md_onstep_velocity + ops.vacf_accumulate (and the copy of a new origin) per step, mean over the run, best of repeats
  vacf_step_ms / vacf_step_sampled_ms   the sum without and with vacf_ms; the ring is full after 64 samples, as above
--sq adds what forces.sample costs when a forces.Scatter samples the structure factors at EVERY step (every = 1; sq: n_max = 4, the
364 vectors of the half space; fqt: 16 lags, a new origin every 4 samples; three types), from a run of its own in which the two
launches are a fourth phase between rebuild and evaluate, where the loop has them:
  sq_rebuild_ms / sq_evaluate_ms / sq_md_ms   the three phases above in that run: their sum, sq_step_ms, is the un-sampled step
  sq_ms             ops.density_modes + ops.sq_accumulate (and the copy of the modes into the ring at a new origin) per step, mean
                    over the run, best of repeats
  sq_modes_ms / sq_products_ms   the same two launches alone, the first and the second (with the copy) — their sum is sq_ms
  sq_step_ms / sq_step_sampled_ms   the sum without and with sq_ms.  The ring holds 4 origins and is full after 16 samples"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_forces import structures  # noqa: E402
from bench_relax import events, make_model  # noqa: E402
from matdeeplearn_amd import forces, ops  # noqa: E402
from matdeeplearn_amd.process import graph as pg  # noqa: E402

MD = dict(dt=1.0, gamma=0.05, kT=2e-5, seed=0)
NPT = dict(pressure=0.0, rate=30.0, max_strain=0.03)


def torch_md_step(pos, vel, force, mass, batch, st, dt, n_steps, gamma, kT, max_disp):
    """ops.md_step from torch ops, in place, no host decision: two segmented sums between elementwise passes, noise from torch.randn"""
    B = st.steps.numel()
    seg = lambda x: torch.zeros(B, dtype=torch.float64, device=pos.device).index_add_(0, batch, x)
    per = lambda x: x[batch].unsqueeze(1)
    m = mass.unsqueeze(1)
    a = force.double() / m
    h = 0.5 * dt
    run = st.status == 0
    v = torch.where(per(st.steps > 0), vel + per(h) * a, vel)
    ekin = 0.5 * seg((m * v * v).sum(1))
    closing = run & (st.steps == n_steps)
    v1 = v + per(h) * a
    x1 = pos + per(h) * v1
    c1, c2 = torch.exp(-gamma * dt), torch.sqrt(-torch.expm1(-2.0 * gamma * dt))
    v2 = torch.where(per(gamma > 0), per(c1) * v1 + per(c2) * torch.sqrt(per(kT) / m) * torch.randn_like(v1), v1)
    x2 = x1 + per(h) * v2
    n_bad = seg((~(((x2 - pos) ** 2).sum(1).sqrt() <= max_disp)).double())
    accept = run & ~closing & (n_bad == 0)
    pos.copy_(torch.where(per(accept), x2, pos))
    vel.copy_(torch.where(per(accept), v2, torch.where(per(run), v, vel)))
    st.ekin.copy_(torch.where(run, ekin, st.ekin))
    st.steps.add_(accept.to(torch.int32))
    st.status.copy_(torch.where(closing, 1, torch.where(run & ~accept, 2, st.status)).to(torch.int32))
    return st


def md_inputs(ff, seed):
    dev, B = ff.positions.device, ff.node_ptr.numel() - 1
    mass = torch.from_numpy(np.random.default_rng(seed).uniform(1.0, 4.0, ff.positions.shape[0])).to(dev)
    per = lambda v: torch.full((B,), v, dtype=torch.float64, device=dev)
    return mass, per(MD["dt"]), per(MD["gamma"]), per(MD["kT"]), torch.arange(B, dtype=torch.int64, device=dev) + MD["seed"]


def md_phases(model, packed, steps, seed, npt=False):
    """one run, every step rebuilt: per-step means (ms) of the three phases, and how many structures a guard stopped; npt: the step
    of forces.md_npt in the place of that of forces.md"""
    ff = forces.ForceField(model, packed, (0.0, 8.0))
    dev, B = ff.positions.device, ff.node_ptr.numel() - 1
    mass, dt, gamma, kT, keys = md_inputs(ff, seed)
    vel = ops.md_velocities(mass, ff.node_ptr, kT, keys)
    state, n_steps = (ops.md_cell_state if npt else ops.md_state)(B, dev), torch.full((B,), steps, dtype=torch.int32, device=dev)
    marks = []
    for _ in range(steps):
        e = events(4)
        e[0].record()
        ff.rebuild()
        e[1].record()
        if npt:
            _, f, strain = ff.evaluate(stress=True, volume_normalised=False)
            e[2].record()
            ops.md_cell_step(ff.positions, vel, ff.cell, f, strain, mass, ff.node_ptr, state, dt, n_steps, NPT["pressure"], NPT["rate"], gamma, kT,
                             keys, max_strain=NPT["max_strain"])
        else:
            _, f = ff.evaluate()
            e[2].record()
            ops.md_step(ff.positions, vel, f, mass, ff.node_ptr, state, dt, n_steps, gamma, kT, keys)
        e[3].record()
        marks.append(e)
    torch.cuda.synchronize()
    return [sum(e[k].elapsed_time(e[k + 1]) for e in marks) / steps for k in range(3)], int((state.steps != steps).sum())


OBSERVE = dict(every=1, rdf=dict(r_max=8.0, nbins=256), msd=dict(n_lags=64, origin_every=4))


def observe_phases(model, packed, steps, seed):
    """md_phases with the sampling of forces.sample at every step as a phase of its own: per-step means (ms) of rebuild, observe,
    evaluate, md"""
    ff = forces.ForceField(model, packed, (0.0, 8.0))
    dev, B = ff.positions.device, ff.node_ptr.numel() - 1
    mass, dt, gamma, kT, keys = md_inputs(ff, seed)
    vel = ops.md_velocities(mass, ff.node_ptr, kT, keys)
    state, n_steps = ops.md_state(B, dev), torch.full((B,), steps, dtype=torch.int32, device=dev)
    obs = forces._Observer(forces.Observe(types=np.asarray(packed["numbers"]) % 3, **OBSERVE), packed, steps)
    obs.start(ff, mass, None, dt, steps, False)
    marks = []
    for it in range(steps):
        e = events(5)
        e[0].record()
        ff.rebuild()
        e[1].record()
        obs.sample(it, ff, state.status)
        e[2].record()
        _, f = ff.evaluate()
        e[3].record()
        ops.md_step(ff.positions, vel, f, mass, ff.node_ptr, state, dt, n_steps, gamma, kT, keys)
        e[4].record()
        marks.append(e)
    torch.cuda.synchronize()
    assert int(obs.state.frames.min()) == steps and int(obs.state.flag.max()) == 0
    return [sum(e[k].elapsed_time(e[k + 1]) for e in marks) / steps for k in range(4)]


VACF = dict(every=1, vacf=dict(n_lags=64, origin_every=4))


def vacf_phases(model, packed, steps, seed):
    """md_phases with the velocity sampling of forces.sample (a forces.Correlate) at every step as a phase of its own, between
    evaluate and md where the loop has it: per-step means (ms) of rebuild, evaluate, vacf, md"""
    ff = forces.ForceField(model, packed, (0.0, 8.0))
    dev, B = ff.positions.device, ff.node_ptr.numel() - 1
    mass, dt, gamma, kT, keys = md_inputs(ff, seed)
    vel = ops.md_velocities(mass, ff.node_ptr, kT, keys)
    state, n_steps = ops.md_state(B, dev), torch.full((B,), steps, dtype=torch.int32, device=dev)
    obs = forces._Observer(forces.Correlate(types=np.asarray(packed["numbers"]) % 3, **VACF), packed, steps)
    obs.start(ff, mass, None, dt, steps, False)
    marks = []
    for it in range(steps):
        e = events(5)
        e[0].record()
        ff.rebuild()
        e[1].record()
        _, f = ff.evaluate()
        e[2].record()
        obs.sample_velocities(it, vel, f, state, dt)
        e[3].record()
        ops.md_step(ff.positions, vel, f, mass, ff.node_ptr, state, dt, n_steps, gamma, kT, keys)
        e[4].record()
        marks.append(e)
    torch.cuda.synchronize()
    assert int(obs.vstate.vacf_count[:, 0].min()) == (steps + 3) // 4
    return [sum(e[k].elapsed_time(e[k + 1]) for e in marks) / steps for k in range(4)]


SQ = dict(every=1, sq=dict(n_max=4, fqt=dict(n_lags=16, origin_every=4)))


def sq_phases(model, packed, steps, seed):
    """md_phases with the structure-factor sampling of forces.sample (a forces.Scatter) at every step as two phases of their own,
    between rebuild and evaluate where the loop has them: per-step means (ms) of rebuild, the modes, the products, evaluate, md"""
    ff = forces.ForceField(model, packed, (0.0, 8.0))
    dev, B = ff.positions.device, ff.node_ptr.numel() - 1
    mass, dt, gamma, kT, keys = md_inputs(ff, seed)
    vel = ops.md_velocities(mass, ff.node_ptr, kT, keys)
    state, n_steps = ops.md_state(B, dev), torch.full((B,), steps, dtype=torch.int32, device=dev)
    obs = forces._Observer(forces.Scatter(types=np.asarray(packed["numbers"]) % 3, **SQ), packed, steps)
    obs.start(ff, mass, None, dt, steps, False)
    st = obs.sstate
    marks = []
    for it in range(steps):
        e = events(6)
        e[0].record()
        ff.rebuild()
        e[1].record()
        # what _Observer.sample does for a Scatter, with an event between the two launches
        s = obs.sample_of[it]
        ops.density_modes(ff.positions, ff.cell, ff.pbc, st, state.status)
        e[2].record()
        if obs.qslot[s] >= 0:
            st.origins[obs.qslot[s]].copy_(st.rho)
        ops.sq_accumulate(obs.qlag[s], st, state.status)
        e[3].record()
        _, f = ff.evaluate()
        e[4].record()
        ops.md_step(ff.positions, vel, f, mass, ff.node_ptr, state, dt, n_steps, gamma, kT, keys)
        e[5].record()
        marks.append(e)
    torch.cuda.synchronize()
    assert int(st.frames.min()) == steps and int(st.flag.max()) == 0 and int(st.fqt_count[:, 0].min()) == (steps + 3) // 4
    return [sum(e[k].elapsed_time(e[k + 1]) for e in marks) / steps for k in range(5)]


def integrator_alone(model, packed, repeats, seed, npt=False):
    ff = forces.ForceField(model, packed, (0.0, 8.0))
    dev, B, N = ff.positions.device, ff.node_ptr.numel() - 1, ff.positions.shape[0]
    _, f, strain = ff.evaluate(stress=True, volume_normalised=False)
    batch = torch.repeat_interleave(torch.arange(B, device=dev), ff.node_ptr[1:] - ff.node_ptr[:-1], output_size=N)
    mass, dt, gamma, kT, keys = md_inputs(ff, seed)
    vel0 = ops.md_velocities(mass, ff.node_ptr, kT, keys)
    state0, n_steps = ops.md_state(B, dev), torch.full((B,), 100, dtype=torch.int32, device=dev)
    # one call on the state every timed call clones: the values of mass, dt, gamma, kT and n_steps are read back here, once, as at
    # the first step of a run (the clones inherit what the state has seen)
    ops.md_step(ff.positions.clone(), vel0.clone(), f, mass, ff.node_ptr, state0, dt, n_steps, gamma, kT, keys)
    state0.steps.fill_(3)                                       # past the first step: the closing kick runs
    zero = 0.0                                                  # a number: no thermostat, nothing to read back

    def timed(step):
        pos, vel, st = ff.positions.clone(), vel0.clone(), state0.clone()
        e = events(2)
        e[0].record()
        step(pos, vel, st)
        e[1].record()
        return e, pos

    fns = (lambda: timed(lambda p, v, s: ops.md_step(p, v, f, mass, ff.node_ptr, s, dt, n_steps, gamma, kT, keys)),
           lambda: timed(lambda p, v, s: ops.md_step(p, v, f, mass, ff.node_ptr, s, dt, n_steps, zero, kT, keys)),
           lambda: timed(lambda p, v, s: torch_md_step(p, v, f, mass, batch, s, dt, n_steps, gamma, kT, 0.5)),
           lambda: timed(lambda p, v, s: torch_md_step(p, v, f, mass, batch, s, dt, n_steps, torch.zeros_like(gamma), kT, 0.5)))
    if npt:
        cstate0 = ops.md_cell_state(B, dev)
        cstate0._checked = dict(state0._checked)
        cstate0.steps.fill_(3)

        def timed_cell():
            pos, vel, cell, st = ff.positions.clone(), vel0.clone(), ff.cell.clone(), cstate0.clone()
            e = events(2)
            e[0].record()
            ops.md_cell_step(pos, vel, cell, f, strain, mass, ff.node_ptr, st, dt, n_steps, NPT["pressure"], NPT["rate"], gamma, kT, keys,
                             max_strain=NPT["max_strain"])
            e[1].record()
            return e, pos

        fns += (timed_cell,)
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
    out = {"md_us": round(best[0] * 1e3, 1), "md_nve_us": round(best[1] * 1e3, 1), "torch_us": round(best[2] * 1e3, 1),
           "max_pos_diff": float((outs[1][0] - outs[3][0]).abs().max()), "md_repeatable": same(outs[0]), "torch_repeatable": same(outs[2])}
    if npt:
        out.update(md_cell_us=round(best[4] * 1e3, 1), md_cell_repeatable=same(outs[4]))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("cgcnn", "schnet"), default="cgcnn")
    ap.add_argument("--graphs", default="64,1024")
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--npt", action="store_true", help="add the step of forces.md_npt to every line")
    ap.add_argument("--observe", action="store_true", help="add the step with forces.sample's sampling at every step to every line")
    ap.add_argument("--vacf", action="store_true", help="add the step with forces.sample's velocity sampling at every step to every line")
    ap.add_argument("--sq", action="store_true", help="add the step with forces.sample's structure-factor sampling at every step to every line")
    a = ap.parse_args()
    model = make_model(a, torch.device("cuda"))
    for B in [int(v) for v in a.graphs.split(",")]:
        packed = pg.pack_structures(structures(B, a.seed))
        md_phases(model, packed, 2, a.seed)                                # warm-up (code objects, allocator)
        best = None
        for _ in range(a.repeats):
            t, stopped = md_phases(model, packed, a.steps, a.seed)
            best = t if best is None else [min(x, y) for x, y in zip(best, t)]
        line = {"model": a.model, "graphs": B, "atoms": int(packed["node_ptr"][-1]), "dim": a.dim, "steps": a.steps,
                "rebuild_ms": round(best[0], 3), "evaluate_ms": round(best[1], 3), "md_ms": round(best[2], 4), "stopped": stopped}
        if a.npt:
            md_phases(model, packed, 2, a.seed, npt=True)
            best = None
            for _ in range(a.repeats):
                t, stopped = md_phases(model, packed, a.steps, a.seed, npt=True)
                best = t if best is None else [min(x, y) for x, y in zip(best, t)]
            line.update(npt_rebuild_ms=round(best[0], 3), npt_evaluate_ms=round(best[1], 3), npt_md_ms=round(best[2], 4), npt_stopped=stopped)
        if a.observe:
            observe_phases(model, packed, 2, a.seed)
            best = None
            for _ in range(a.repeats):
                t = observe_phases(model, packed, a.steps, a.seed)
                best = t if best is None else [min(x, y) for x, y in zip(best, t)]
            plain = best[0] + best[2] + best[3]
            line.update(obs_rebuild_ms=round(best[0], 3), observe_ms=round(best[1], 4), obs_evaluate_ms=round(best[2], 3),
                        obs_md_ms=round(best[3], 4), step_ms=round(plain, 3), step_observed_ms=round(plain + best[1], 3))
        if a.vacf:
            vacf_phases(model, packed, 2, a.seed)
            best = None
            for _ in range(a.repeats):
                t = vacf_phases(model, packed, a.steps, a.seed)
                best = t if best is None else [min(x, y) for x, y in zip(best, t)]
            plain = best[0] + best[1] + best[3]
            line.update(vacf_rebuild_ms=round(best[0], 3), vacf_evaluate_ms=round(best[1], 3), vacf_ms=round(best[2], 4),
                        vacf_md_ms=round(best[3], 4), vacf_step_ms=round(plain, 3), vacf_step_sampled_ms=round(plain + best[2], 3))
        if a.sq:
            sq_phases(model, packed, 2, a.seed)
            best = None
            for _ in range(a.repeats):
                t = sq_phases(model, packed, a.steps, a.seed)
                best = t if best is None else [min(x, y) for x, y in zip(best, t)]
            plain = best[0] + best[3] + best[4]
            line.update(sq_rebuild_ms=round(best[0], 3), sq_modes_ms=round(best[1], 4), sq_products_ms=round(best[2], 4),
                        sq_ms=round(best[1] + best[2], 4), sq_evaluate_ms=round(best[3], 3), sq_md_ms=round(best[4], 4),
                        sq_step_ms=round(plain, 3), sq_step_sampled_ms=round(plain + best[1] + best[2], 3))
        line.update(integrator_alone(model, packed, a.repeats, a.seed, a.npt))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
