#!/usr/bin/env python3
"""Forces from positions: forces.energy_and_forces on a batch of bulk-like structures, fused distance path vs the general [E, G] path.

  python tools/bench_forces.py [--model cgcnn|schnet] [--graphs 8192] [--dim 64] [--dtypes fp32,bf16] [--repeats 5] [--seed 0]

Structures are drawn with the size recipe of process.synthetic_bulk (n ~ lognormal(ln 20, 0.7) clipped to [1, 200], cubic periodic
cell at density 0.05, uniform positions, Z ~ U[1, 89]); the model is a seeded CGCNN (dim1 = dim2 = --dim, 4 conv layers) or, with
--model schnet, a seeded SchNet (dim1 = dim2 = dim3 = --dim, 3 interaction blocks) in eval mode.  The fused and the general
runs alternate, so both see the same machine state.
Reported per dtype, one JSON line:
  fused_ms / general_ms   one energy_and_forces call end to end (packing on the host included), device events, best of repeats
  max_abs_diff_rel        max |F_fused - F_general| / max |F|
The per-layer kernel times (cgconv_de_kernel / cfconv_de_*_kernel in both epilogues, rbf_bwd_kernel, edge_geom_*) come from a kernel trace of this
script, e.g.  rocprofv3 --kernel-trace --stats -- python tools/bench_forces.py --repeats 2  (a process of its own)."""
import argparse
import json
import os
import sys
import types

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matdeeplearn_amd import forces, models  # noqa: E402
from matdeeplearn_amd.process import graph as pg  # noqa: E402


def structures(n_graphs, seed):
    rng = np.random.default_rng(seed)
    sizes = np.clip(np.rint(np.exp(rng.normal(np.log(20.0), 0.7, n_graphs))), 1, 200).astype(int)
    out = []
    for n in sizes:
        side = (n / 0.05) ** (1.0 / 3.0)
        out.append(dict(positions=rng.uniform(0.0, side, size=(n, 3)), numbers=rng.integers(1, 90, size=n),
                        cell=np.diag([side] * 3), pbc=np.array([True, True, True])))
    return out


class DS:
    num_features, num_edge_features = 114, 50

    def __getitem__(self, i):
        return types.SimpleNamespace(y=torch.tensor(0.0), u=torch.zeros(1, 3))


def timed(fns, repeats):
    """best-of-repeats time and last result of every callable, the callables taking turns"""
    best, out = [None] * len(fns), [None] * len(fns)
    for _ in range(repeats):
        for k, fn in enumerate(fns):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out[k] = fn()
            e1.record()
            torch.cuda.synchronize()
            t = e0.elapsed_time(e1)
            best[k] = t if best[k] is None else min(best[k], t)
    return best, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("cgcnn", "schnet"), default="cgcnn")
    ap.add_argument("--graphs", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    dev = torch.device("cuda")
    packed = pg.pack_structures(structures(a.graphs, a.seed))
    for dt in a.dtypes.split(","):
        torch.manual_seed(a.seed)
        if a.model == "schnet":
            model = models.SchNet(DS(), dim1=a.dim, dim2=a.dim, dim3=a.dim, gc_count=3, post_fc_count=1, compute_dtype=dt).to(dev).eval()
        else:
            model = models.CGCNN(DS(), dim1=a.dim, dim2=a.dim, gc_count=4, post_fc_count=1, compute_dtype=dt).to(dev).eval()
        run = lambda fused: forces.energy_and_forces(model, packed, (0.0, 8.0), fused=fused)
        run(True), run(False)                                                  # warm-up (code objects, allocator)
        (t_f, t_g), ((_, f_f, _), (_, f_g, _)) = timed([lambda: run(True), lambda: run(False)], a.repeats)
        print(json.dumps({"model": a.model, "dtype": dt, "graphs": a.graphs, "atoms": int(packed["node_ptr"][-1]), "dim": a.dim,
                          "fused_ms": round(t_f, 3), "general_ms": round(t_g, 3),
                          "max_abs_diff_rel": float((f_f - f_g).abs().max() / f_f.abs().max())}), flush=True)


if __name__ == "__main__":
    main()
