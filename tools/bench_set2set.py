"""Set2Set readout: fused kernels (ops.set2set, csrc/set2set.hip) against the composed path (torch's LSTM + gathers / segment
reductions, `ops.configure(set2set_fused=False)`), forward + backward of the readout alone, and the whole CGCNN training step with
pool = "set2set" at the reference's batch size, eager against HIP-graph replay.

Timing: device events around one forward + backward, median and spread over --reps repeats after --warmup warm-up calls, the two
paths alternating inside one process.  Segment sizes are bulk-like (uniform 1..200 nodes per graph).  One JSON line per point.

    python tools/bench_set2set.py [--reps 30] [--warmup 5] [--graphs 100,8192] [--widths 64,100] [--no-step]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matdeeplearn_amd import models, nn as mnn, ops  # noqa: E402
import _ab  # noqa: E402

_ab.apply()      # (tools/_ab.py: MDL_HIP_LIB / MDL_OPS of the A/B scripts -> explicit calls)


def _median_ms(events):
    ts = sorted(a.elapsed_time(b) for a, b in events)
    return ts[len(ts) // 2], ts[0], ts[-1]


def _timed(fn, store):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    store.append((a, b))


def readout_point(S, C, dtype, reps, warmup, dev):
    rng = np.random.default_rng(S + C)
    sizes = rng.integers(1, 201, size=S)
    N = int(sizes.sum())
    batch = torch.from_numpy(np.repeat(np.arange(S), sizes)).to(dev)
    gen = torch.Generator().manual_seed(C)
    x = torch.randn(N, C, generator=gen).to(dev).to(dtype).requires_grad_(True)
    gout = torch.randn(S, 2 * C, generator=gen).to(dev)
    torch.manual_seed(1)
    m = mnn.Set2Set(C, processing_steps=3).to(dev)

    def step():
        m.zero_grad(set_to_none=True)
        x.grad = None
        (m(x, batch, S) * gout).sum().backward()

    ev = {False: [], True: []}
    out = {}
    for fused in (False, True):
        prev = ops.configure(set2set_fused=fused)
        for _ in range(warmup):
            step()
        out[fused] = (m(x, batch, S).detach().clone(), x.grad.detach().float().clone())
        ops.configure(**prev)
    torch.cuda.synchronize()
    for _ in range(reps):
        for fused in (False, True):
            prev = ops.configure(set2set_fused=fused)
            _timed(step, ev[fused])
            ops.configure(**prev)
    torch.cuda.synchronize()
    (c_med, c_lo, c_hi), (f_med, f_lo, f_hi) = _median_ms(ev[False]), _median_ms(ev[True])
    scale = float(out[False][0].abs().max())
    return dict(point="readout_fwd_bwd", graphs=S, nodes=N, C=C, dtype=str(dtype).split(".")[-1], reps=reps,
                composed_ms=round(c_med, 4), composed_min_max=[round(c_lo, 4), round(c_hi, 4)],
                fused_ms=round(f_med, 4), fused_min_max=[round(f_lo, 4), round(f_hi, 4)], speedup=round(c_med / f_med, 2),
                out_diff_rel=float((out[True][0] - out[False][0]).abs().max()) / scale,
                dx_diff_rel=float((out[True][1] - out[False][1]).abs().max()) / (float(out[False][1].abs().max()) + 1e-30))


def step_point(reps, warmup, dev, B=100):
    """whole training step of CGCNN-64 with pool = "set2set" at batch B: eager (both readout paths) and replayed"""
    import copy
    from matdeeplearn_amd.process import synthetic_bulk
    from matdeeplearn_amd.training import GraphedStep, make_optimizer
    ds = synthetic_bulk(4 * B, seed=0).to(dev)
    rng = np.random.default_rng(0)
    ids = [rng.choice(len(ds), size=B, replace=False) for _ in range(reps + warmup)]
    torch.manual_seed(0)
    m0 = models.CGCNN(ds, dim1=64, dim2=64, gc_count=4, post_fc_count=3, pool="set2set", compute_dtype="bf16").to(dev)
    res = dict(point="cgcnn64_set2set_step", batch=B, reps=reps)

    def eager(fused):
        m = copy.deepcopy(m0).train()
        opt = make_optimizer(m.parameters(), "AdamW", lr=0.002)
        prev = ops.configure(set2set_fused=fused)
        ev = []

        def one(k):
            batch = ds.collate(ids[k], edge_dtype=torch.bfloat16, x_dtype=torch.bfloat16)
            opt.zero_grad(set_to_none=True)
            with ops.zero_arena(dev):
                ops.backward(torch.nn.functional.l1_loss(m(batch), batch.y))
            opt.step()
        for k in range(warmup):
            one(k)
        torch.cuda.synchronize()
        for k in range(warmup, warmup + reps):
            _timed(lambda: one(k), ev)
        torch.cuda.synchronize()
        ops.configure(**prev)
        return _median_ms(ev)

    for name, fused in (("eager_composed", False), ("eager_fused", True)):
        med, lo, hi = eager(fused)
        res[name + "_ms"], res[name + "_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    m = copy.deepcopy(m0)
    gs = GraphedStep(ds, m, make_optimizer(m.parameters(), "AdamW", lr=0.002, capturable=True), B, compute_dtype=torch.bfloat16)
    ev = []
    for k in range(warmup):
        gs.step(ids[k])
    torch.cuda.synchronize()
    for k in range(warmup, warmup + reps):
        _timed(lambda: gs.step(ids[k]), ev)
    torch.cuda.synchronize()
    med, lo, hi = _median_ms(ev)
    res["replayed_fused_ms"], res["replayed_fused_min_max"] = round(med, 4), [round(lo, 4), round(hi, 4)]
    res["replays"], res["eager_steps"] = gs.replays, gs.eager_steps
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--graphs", default="100,8192")
    ap.add_argument("--widths", default="64,100")
    ap.add_argument("--no-step", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_set2set: needs a HIP device (no CPU timing)")
    if a.reps < 20:
        raise SystemExit("bench_set2set: at least 20 repeats")
    dev = torch.device("cuda:0")
    for S in [int(v) for v in a.graphs.split(",")]:
        for C in [int(v) for v in a.widths.split(",")]:
            for dtype in (torch.float32, torch.bfloat16):
                print(json.dumps(readout_point(S, C, dtype, a.reps, a.warmup, dev)), flush=True)
    if not a.no_step:
        print(json.dumps(step_point(a.reps, a.warmup, dev)), flush=True)


if __name__ == "__main__":
    main()
