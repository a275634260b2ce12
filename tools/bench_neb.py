#!/usr/bin/env python3
"""Nudged-elastic-band step on the device: what one step of forces.neb costs, phase by phase, and ops.neb_step against the same step
composed from torch ops.

  python tools/bench_neb.py [--model cgcnn|schnet] [--bands 8,128] [--images 7] [--dim 64] [--steps 20] [--repeats 5] [--seed 0]

Structures and model as tools/bench_relax.py takes them; every band runs from a structure to a copy displaced by uniform noise of
0.3 A, --images images each (forces.interpolate_band); dt = 3, fmax = 0, spring = 0.01, climbing from the first step (an untrained
model's forces are of order 1e-3 per A).  One JSON line per batch size:
  rebuild_ms / evaluate_ms / neb_ms   device events around ForceField.rebuild(), ForceField.evaluate() and ops.neb_step of every
                                      step of a --steps long run with rebuild_every = 1, mean per step, best of --repeats runs
  neb_us / torch_us   the step alone on the forces of the first evaluation: the two HIP launches of ops.neb_step against
                    torch_neb_step below (the band force from gathers, batched 3x3 products and index_add_ / scatter_reduce_ over
                    the images, then bench_relax.torch_fire_step over the bands), taking turns, best of repeats, on clones of one
                    state
  max_pos_diff      largest difference between the positions the two produce in that one step
  neb_repeatable / torch_repeatable   whether 5 runs from the same inputs gave the same bits"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from bench_forces import structures  # noqa: E402
from bench_relax import events, make_model, torch_fire_step  # noqa: E402
from matdeeplearn_amd import forces, ops  # noqa: E402

NEB = dict(dt=3.0, fmax=0.0, spring=0.01, noise=0.3)
CONST = dict(ops.FIRE_CONSTANTS, dt_max=30.0)


def make_bands(n_bands, n_images, seed):
    rng = np.random.default_rng(seed + 1)
    out = []
    for s in structures(n_bands, seed):
        final = dict(s, positions=s["positions"] + rng.uniform(-NEB["noise"], NEB["noise"], s["positions"].shape))
        out.append(forces.interpolate_band(s, final, n_images))
    return out


class Layout:
    """index tensors of a batch of bands for torch_neb_step: per atom its image, its band and its image's atom count; per image its
    band and whether it is a first / last image"""

    def __init__(self, state):
        ip, bp = state.image_ptr, state.band_ptr
        dev, I, B, N = ip.device, ip.numel() - 1, bp.numel() - 1, state.fixed.numel()
        cnt = ip[1:] - ip[:-1]
        self.img = torch.repeat_interleave(torch.arange(I, device=dev), cnt, output_size=N)
        self.cnt = cnt[self.img]
        self.img_band = torch.repeat_interleave(torch.arange(B, device=dev), bp[1:] - bp[:-1], output_size=I)
        self.band = self.img_band[self.img]
        self.first = torch.zeros(I, dtype=torch.bool, device=dev)
        self.last = torch.zeros(I, dtype=torch.bool, device=dev)
        self.first[bp[:-1]] = True
        self.last[bp[1:] - 1] = True
        self.I, self.B, self.N = I, B, N


def torch_neb_force(pos, force, energy, cell, pbc, fixed, spring, climb, L):
    """the band force of csrc/neb.hip from torch ops (every cell with a volume): (band_force fp32, F.t^, |t-|, climber)"""
    dev, idx = pos.device, torch.arange(L.N, device=pos.device)
    inv = torch.linalg.inv(cell)
    per = torch.stack([(pbc >> k) & 1 for k in range(3)], 1).double()

    def wrap(d):
        f = torch.bmm(d.unsqueeze(1), inv[L.img]).squeeze(1)
        f = f - torch.round(f) * per[L.img]
        return torch.bmm(f.unsqueeze(1), cell[L.img]).squeeze(1)

    interior = ~L.first & ~L.last
    tp = wrap(pos[(idx + L.cnt).clamp(max=L.N - 1)] - pos) * (~L.last)[L.img].unsqueeze(1)
    tm = wrap(pos - pos[(idx - L.cnt).clamp(min=0)]) * (~L.first)[L.img].unsqueeze(1)
    free = (fixed == 0).unsqueeze(1)
    F = force.double() * free
    seg = lambda x: torch.zeros(L.I, dtype=torch.float64, device=dev).index_add_(0, L.img, x)
    pp, mm, pm, fp, fm = seg((tp * tp).sum(1)), seg((tm * tm).sum(1)), seg((tp * tm).sum(1)), seg((F * tp).sum(1)), seg((F * tm).sum(1))
    E = energy.double()
    En, Ep = torch.roll(E, -1), torch.roll(E, 1)
    up, down = (En > E) & (E > Ep), (En < E) & (E < Ep)
    dn, dp = (En - E).abs(), (Ep - E).abs()
    hi, lo = torch.maximum(dn, dp), torch.minimum(dn, dp)
    one, zero = torch.ones_like(E), torch.zeros_like(E)
    ca = torch.where(up, one, torch.where(down, zero, torch.where(En > Ep, hi, lo)))
    cb = torch.where(up, zero, torch.where(down, one, torch.where(En > Ep, lo, hi)))
    t2 = ca * ca * pp + 2.0 * ca * cb * pm + cb * cb * mm
    ok = interior & (t2 > 0)
    lt = torch.where(ok, t2, one).sqrt()
    ft = torch.where(ok, (ca * fp + cb * fm) / lt, zero)
    e_in = torch.where(interior, E, torch.full_like(E, float("-inf")))
    top = torch.full((L.B,), float("-inf"), dtype=torch.float64, device=dev).scatter_reduce_(0, L.img_band, e_in, "amax")
    cand = torch.where(interior & (e_in == top[L.img_band]), torch.arange(L.I, device=dev), torch.full_like(L.img_band, L.I))
    climber = torch.full((L.B,), L.I, dtype=torch.int64, device=dev).scatter_reduce_(0, L.img_band, cand, "amin")
    climber = torch.where((climber < L.I) & (climb != 0), climber, torch.full_like(climber, -1))
    climbs = torch.arange(L.I, device=dev) == climber[L.img_band]
    g = torch.where(ok, torch.where(climbs, -2.0 * ft, spring[L.img_band] * (pp.sqrt() - mm.sqrt()) - ft) / lt, zero)
    tau = ca[L.img].unsqueeze(1) * tp + cb[L.img].unsqueeze(1) * tm
    out = (F + g[L.img].unsqueeze(1) * tau) * interior[L.img].unsqueeze(1)
    return out.float(), ft, mm.sqrt(), climber.to(torch.int32)


def torch_neb_step(pos, vel, force, energy, cell, pbc, st, fmax, spring, climb, L, c):
    """ops.neb_step from torch ops, in place, no host decision"""
    bf, ft, seg_len, climber = torch_neb_force(pos, force, energy, cell, pbc, st.fixed, spring, climb, L)
    st.band_force.copy_(bf)
    st.tangent_force.copy_(ft)
    st.seg_len.copy_(seg_len)
    st.climber.copy_(climber)
    return torch_fire_step(pos, vel, bf, L.band, st, fmax, st.fixed, c)


def band_inputs(ff, bands):
    dev = ff.positions.device
    band_ptr = torch.from_numpy(np.concatenate([[0], np.cumsum([len(b) for b in bands])]).astype(np.int64)).to(dev)
    B = band_ptr.numel() - 1
    per = lambda v: torch.full((B,), v, dtype=torch.float64, device=dev)
    return band_ptr, per(NEB["fmax"]), per(NEB["spring"]), torch.ones(B, dtype=torch.uint8, device=dev)


def neb_phases(model, bands, steps):
    """one run, every step rebuilt: per-step means (ms) of the three phases"""
    ff = forces.ForceField(model, [s for b in bands for s in b], (0.0, 8.0))
    band_ptr, fmax, spring, climb = band_inputs(ff, bands)
    state = ops.neb_state(ff.node_ptr, band_ptr, dt=NEB["dt"])
    vel = torch.zeros_like(ff.positions)
    marks = []
    for _ in range(steps):
        e = events(4)
        e[0].record()
        ff.rebuild()
        e[1].record()
        energy, f = ff.evaluate()
        e[2].record()
        ops.neb_step(ff.positions, vel, f, energy, ff.cell, ff.pbc, state, fmax, spring, climb, **CONST)
        e[3].record()
        marks.append(e)
    torch.cuda.synchronize()
    return [sum(e[k].elapsed_time(e[k + 1]) for e in marks) / steps for k in range(3)]


def step_alone(model, bands, repeats):
    ff = forces.ForceField(model, [s for b in bands for s in b], (0.0, 8.0))
    energy, f = ff.evaluate()
    band_ptr, fmax, spring, climb = band_inputs(ff, bands)
    state0 = ops.neb_state(ff.node_ptr, band_ptr, dt=NEB["dt"])
    state0.steps.fill_(3)                                       # past the first step: the mixing runs
    state0.n_pos.fill_(2)
    L = Layout(state0)
    bf0 = torch_neb_force(ff.positions, f, energy, ff.cell, ff.pbc, state0.fixed, spring, climb, L)[0]
    vel0 = 0.7 * bf0.double()                                   # F.v > 0

    def timed(step):
        pos, vel, st = ff.positions.clone(), vel0.clone(), state0.clone()
        e = events(2)
        e[0].record()
        step(pos, vel, st)
        e[1].record()
        return e, pos

    fns = (lambda: timed(lambda p, v, s: ops.neb_step(p, v, f, energy, ff.cell, ff.pbc, s, fmax, spring, climb, **CONST)),
           lambda: timed(lambda p, v, s: torch_neb_step(p, v, f, energy, ff.cell, ff.pbc, s, fmax, spring, climb, L, CONST)))
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
    return {"neb_us": round(best[0] * 1e3, 1), "torch_us": round(best[1] * 1e3, 1), "max_pos_diff": float((outs[0][0] - outs[1][0]).abs().max()),
            "neb_repeatable": same(outs[0]), "torch_repeatable": same(outs[1])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("cgcnn", "schnet"), default="cgcnn")
    ap.add_argument("--bands", default="8,128")
    ap.add_argument("--images", type=int, default=7)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    model = make_model(a, torch.device("cuda"))
    for B in [int(v) for v in a.bands.split(",")]:
        bands = make_bands(B, a.images, a.seed)
        neb_phases(model, bands, 2)                                         # warm-up (code objects, allocator)
        best = None
        for _ in range(a.repeats):
            t = neb_phases(model, bands, a.steps)
            best = t if best is None else [min(x, y) for x, y in zip(best, t)]
        line = {"model": a.model, "bands": B, "images": B * a.images, "atoms": int(sum(len(s["positions"]) for b in bands for s in b)),
                "dim": a.dim, "steps": a.steps, "rebuild_ms": round(best[0], 3), "evaluate_ms": round(best[1], 3), "neb_ms": round(best[2], 4)}
        line.update(step_alone(model, bands, a.repeats))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
