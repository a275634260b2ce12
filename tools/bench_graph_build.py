#!/usr/bin/env python3
"""Graph construction on the device vs the host: process.from_structures(device="cuda") against the host builder.

  python tools/bench_graph_build.py [--shapes bulk,mof] [--host-subset 400] [--repeats 3] [--seed 0]

Datasets are generated from a seed with the size recipes of process.synthetic_bulk (46,744 graphs, n ~ lognormal(ln 20, 0.7)
clipped to [1, 200], density 0.05) and process.synthetic_mof (18,000 graphs, lognormal(ln 100, 0.5) clipped to [20, 500],
density 0.03), but as general from_structures input: structure dicts with a periodic cubic cell, uniform positions, Z ~ U[1, 89].
Reported per shape:
  device_wall_s     from_structures(device=...) end to end: packing, upload, kernels, copy back, node features (best of repeats)
  kernel_ms         the HIP launches alone (ops._build_graphs_launch between device events; inputs already on the device)
  host_s_extrap     the host builder on the first --host-subset structures (a random sample), scaled to the whole dataset
  equal_on_subset   the device dataset equals the host one on that subset (every field, bitwise)
One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from matdeeplearn_amd import ops  # noqa: E402
from matdeeplearn_amd.process import from_structures, graph as pg  # noqa: E402

SHAPES = {"bulk": dict(n_graphs=46744, density=0.05, mean_atoms=20.0, sigma=0.7, min_atoms=1, max_atoms=200),
          "mof": dict(n_graphs=18000, density=0.03, mean_atoms=100.0, sigma=0.5, min_atoms=20, max_atoms=500)}
FIELDS = ("node_ptr", "edge_ptr", "x", "z", "src", "tgt", "dist", "dist_norm", "in_deg", "lrowptr")


def structures(shape, seed):
    c = SHAPES[shape]
    rng = np.random.default_rng(seed)
    sizes = np.clip(np.rint(np.exp(rng.normal(np.log(c["mean_atoms"]), c["sigma"], c["n_graphs"]))), c["min_atoms"],
                    c["max_atoms"]).astype(int)
    out = []
    for n in sizes:
        side = (n / c["density"]) ** (1.0 / 3.0)
        out.append(dict(positions=rng.uniform(0.0, side, size=(n, 3)), numbers=rng.integers(1, 90, size=n),
                        cell=np.diag([side] * 3), pbc=np.array([True, True, True])))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="bulk,mof")
    ap.add_argument("--host-subset", type=int, default=400)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--radius", type=float, default=8.0)
    ap.add_argument("--max-neighbors", type=int, default=12)
    a = ap.parse_args()
    dev = torch.device("cuda")
    r, k = a.radius, a.max_neighbors
    for shape in a.shapes.split(","):
        structs = structures(shape, a.seed)
        G = len(structs)
        ys, ids = np.zeros((G, 1), dtype=np.float32), [str(i) for i in range(G)]
        from_structures(structs[:64], ys[:64], ids[:64], r, k, device=dev)                     # warm-up (code objects)
        walls = []
        for _ in range(a.repeats):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ds = from_structures(structs, ys, ids, r, k, device=dev)
            walls.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        p = pg.pack_structures(structs)
        pack_s = time.perf_counter() - t0
        args = [torch.from_numpy(p[f]).to(dev) for f in ("pos", "node_ptr", "cell", "pbc")]
        kernel = []
        for _ in range(a.repeats):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            ops._build_graphs_launch(*args, G, r, k)
            e1.record()
            torch.cuda.synchronize()
            kernel.append(e0.elapsed_time(e1))
        m = min(a.host_subset, G)
        t0 = time.perf_counter()
        host = from_structures(structs[:m], ys[:m], ids[:m], r, k)
        host_sub = time.perf_counter() - t0
        sub = from_structures(structs[:m], ys[:m], ids[:m], r, k, device=dev)
        equal = all(np.array_equal(np.asarray(getattr(host, f)), np.asarray(getattr(sub, f))) for f in FIELDS)
        pairs = int((np.diff(p["node_ptr"]).astype(np.int64) ** 2).sum())
        print(json.dumps({"shape": shape, "graphs": G, "atoms": int(p["node_ptr"][-1]), "edges": ds.num_edges,
                          "ordered_pairs": pairs, "device_wall_s": round(min(walls), 4),
                          "device_wall_all_s": [round(w, 4) for w in walls], "pack_s": round(pack_s, 4),
                          "kernel_ms": round(min(kernel), 3), "kernel_all_ms": [round(x, 3) for x in kernel],
                          "host_subset": m, "host_subset_s": round(host_sub, 3),
                          "host_s_extrap": round(host_sub / m * G, 2),
                          "host_ms_per_structure": round(1e3 * host_sub / m, 3), "equal_on_subset": bool(equal)}), flush=True)


if __name__ == "__main__":
    main()
