#!/usr/bin/env python3
"""Forces from positions: forces.energy_and_forces on a batch of bulk-like structures, fused distance path vs the general [E, G] path.

  python tools/bench_forces.py [--model cgcnn|schnet|megnet|mpnn] [--graphs 8192] [--dim 64] [--dtypes fp32,bf16] [--repeats 5] [--seed 0]
  python tools/bench_forces.py --kernel [--edges 2600000] [--widths 64,100] [--dtypes fp32,bf16] [--repeats 20]
  python tools/bench_forces.py --stress [--model ...] [--graphs 8192] [--dtypes fp32] [--repeats 5] [--no-trace]

Structures are drawn with the size recipe of process.synthetic_bulk (n ~ lognormal(ln 20, 0.7) clipped to [1, 200], cubic periodic
cell at density 0.05, uniform positions, Z ~ U[1, 89]); the model is a seeded CGCNN (dim1 = dim2 = --dim, 4 conv layers) or, with
--model schnet, a seeded SchNet (dim1 = dim2 = dim3 = --dim, 3 interaction blocks), with --model megnet / mpnn a seeded MEGNet /
MPNN (dim1 = dim2 = dim3 = --dim, 3 layers) in eval mode.  The fused and the general runs alternate, so both see the same
machine state.
Reported per dtype, one JSON line:
  fused_ms / general_ms   one energy_and_forces call end to end (packing on the host included), device events, best of repeats
  max_abs_diff_rel        max |F_fused - F_general| / max |F|
The per-layer kernel times (cgconv_de_kernel / cfconv_de_*_kernel in both epilogues, rbf_bwd_kernel, edge_geom_*) come from a kernel trace of this
script, e.g.  rocprofv3 --kernel-trace --stats -- python tools/bench_forces.py --repeats 2  (a process of its own).
--kernel: the first-edge-layer distance gradient alone (csrc/linear_de.hip, masked form: g and the layer's ReLU output are read)
against the pair it replaces — the layer's input gradient dx = (g * mask) W into [E, G], then mdl_rbf_expand_bwd — on random
operands, alternating, one JSON line per (dtype, width): fused_us / pair_us (best of repeats, device events) and the achieved
bytes/s on the kernel's compulsory traffic E (2 M s + 8).
--stress: forces.energy_forces_stress and forces.energy_and_forces on the usual batch, alternating, one JSON line per dtype:
stress_ms / forces_ms (best of repeats, device events), their difference, and strain_op_us — one ops.edge_strain_grad call on
the batch's own edge geometry (device events, best of repeats: the operator with its allocations and its launch, not the kernel
alone; the kernel's own time is avg_us of the trace below, against a compulsory traffic of 24 B per edge).  Then, unless --no-trace, the
same run once more as a child process under  rocprofv3 --kernel-trace --stats  (a run of its own: tracing and timing do not
share a process), from whose kernel statistics the share of the edge_strain kernels in the device time is printed."""
import argparse
import json
import os
import re
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


def kernel_bench(a):
    from matdeeplearn_amd import _lib, ops
    dev = torch.device("cuda")
    E, G = a.edges, 50
    offs, coeff = ops.rbf_offsets(0.0, 1.0, G, dev), ops.rbf_coeff(0.0, 1.0, 0.2)
    for dt in a.dtypes.split(","):
        dtype = {"fp32": torch.float32, "bf16": torch.bfloat16}[dt]
        for M in [int(v) for v in a.widths.split(",")]:
            gen = torch.Generator(device=dev).manual_seed(a.seed)
            g = torch.randn(E, M, device=dev, generator=gen).to(dtype)
            y = torch.relu(torch.randn(E, M, device=dev, generator=gen)).to(dtype)
            w = (torch.randn(M, G, device=dev, generator=gen) * 0.3).to(dtype)
            d = torch.rand(E, device=dev, generator=gen)
            dd = torch.empty(E, device=dev)

            def pair():
                if ops._dx_hip_ok(g, w):
                    dx = ops._dx_hip(g, w, (1, y))                      # the mask in the streaming kernel's staging
                else:
                    dx = torch.ops.aten.threshold_backward(g, y, 0) @ w
                _lib.check(_lib.lib().mdl_rbf_expand_bwd(_lib.ptr(dx), G, _lib.dtype_code(dx), _lib.ptr(d), _lib.ptr(offs), coeff,
                                                         _lib.ptr(dd), E, G, _lib.stream()), "mdl_rbf_expand_bwd")
                return dd.clone()

            fused = lambda: ops.linear_dist_grad(g, w, d, act_y=y, resolution=G)
            fused(), pair()
            (t_f, t_p), (r_f, r_p) = timed([fused, pair], a.repeats)
            nbytes = E * (2 * M * g.element_size() + 8)
            print(json.dumps({"kernel": "linear_rbf_dist_grad", "dtype": dt, "edges": E, "M": M, "G": G, "fused_us": round(t_f * 1e3, 1),
                              "pair_us": round(t_p * 1e3, 1), "fused_TBps": round(nbytes / (t_f * 1e-3) / 1e12, 3),
                              "max_abs_diff_rel": float((r_f - r_p).abs().max() / r_f.abs().max())}), flush=True)


def stress_bench(a):
    from matdeeplearn_amd import ops
    dev = torch.device("cuda")
    packed = pg.pack_structures(structures(a.graphs, a.seed))
    for dt in a.dtypes.split(","):
        torch.manual_seed(a.seed)
        model = make_model(a, dt, dev)
        with_stress = lambda: forces.energy_forces_stress(model, packed, (0.0, 8.0))
        without = lambda: forces.energy_and_forces(model, packed, (0.0, 8.0))
        with_stress(), without()
        (t_s, t_f), ((_, f_s, stress, _), (_, f_f, _)) = timed([with_stress, without], a.repeats)
        # the reduction alone, on the geometry of this batch
        t = {k: torch.from_numpy(np.asarray(packed[k])).to(dev) for k in ("pos", "node_ptr", "cell", "pbc")}
        edge_ptr, src, tgt, _, _ = ops.build_graphs(t["pos"], t["node_ptr"], t["cell"], t["pbc"], 8.0, 12)
        dist, u = ops.edge_vectors(t["pos"], t["node_ptr"], t["cell"], t["pbc"], src, tgt, edge_ptr=edge_ptr, return_unit=True)
        shift = torch.repeat_interleave(t["node_ptr"][:-1], edge_ptr[1:] - edge_ptr[:-1], output_size=src.numel()).to(torch.int32)
        N, E = t["pos"].shape[0], src.numel()
        csr = ops.EdgeCSR(ops.csr_rowptr((tgt + shift).contiguous(), N), (src + shift).contiguous(), (tgt + shift).contiguous(), None, N, E)
        g = torch.randn(E, device=dev)
        kernel = lambda: ops.edge_strain_grad(g, dist, u, t["node_ptr"], csr=csr)
        kernel()
        (t_k,), _ = timed([kernel], max(a.repeats, 20))
        print(json.dumps({"model": a.model, "dtype": dt, "graphs": a.graphs, "atoms": N, "edges": E, "dim": a.dim,
                          "stress_ms": round(t_s, 3), "forces_ms": round(t_f, 3), "stress_minus_forces_ms": round(t_s - t_f, 3),
                          "strain_op_us": round(t_k * 1e3, 1),
                          "forces_max_abs_diff_rel": float((f_s - f_f).abs().max() / f_f.abs().max()), "stress_finite": bool(torch.isfinite(stress).all())}), flush=True)
    a.edges_seen = E
    if not a.no_trace:
        kernel_share(a)


def kernel_share(a):
    """the same --stress run as a child process under rocprofv3; share of the edge_strain kernels from its kernel statistics"""
    import csv
    import glob
    import shutil
    import subprocess
    import tempfile
    prof = shutil.which("rocprofv3") or "/opt/rocm/bin/rocprofv3"
    if not os.path.exists(prof):
        print(json.dumps({"trace": "rocprofv3 not found"}), flush=True)
        return
    out = tempfile.mkdtemp(prefix="bench_forces_trace_")
    try:
        cmd = [prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "--", sys.executable, os.path.abspath(__file__), "--stress", "--no-trace",
               "--model", a.model, "--graphs", str(a.graphs), "--dim", str(a.dim), "--dtypes", a.dtypes, "--repeats", "2", "--seed", str(a.seed)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        rows = []
        for f in glob.glob(os.path.join(out, "**", "*kernel_stats*.csv"), recursive=True):
            rows += list(csv.DictReader(open(f)))
        if r.returncode != 0 or not rows:
            found = [os.path.relpath(f, out) for f in glob.glob(os.path.join(out, "**", "*"), recursive=True) if os.path.isfile(f)]
            print(json.dumps({"trace": "no kernel statistics (exit %d)" % r.returncode, "files": found[:20], "tail": r.stdout[-400:]}), flush=True)
            return
        total = sum(float(x["TotalDurationNs"]) for x in rows)
        mine = [x for x in rows if "edge_strain" in x["Name"]]
        kname = lambda full: re.search(r"edge_strain\w*", full).group(0)
        print(json.dumps({"trace_kernels": {kname(x["Name"]): {"calls": int(x["Calls"]), "avg_us": round(float(x["TotalDurationNs"]) / int(x["Calls"]) / 1e3, 2)}
                                            for x in mine},
                          "edge_strain_GBps": {kname(x["Name"]): round(24 * a.edges_seen / (float(x["TotalDurationNs"]) / int(x["Calls"])), 1)
                                               for x in mine if "finish" not in x["Name"] and a.edges_seen},
                          "edge_strain_share_of_device_time": round(sum(float(x["TotalDurationNs"]) for x in mine) / total, 5)}), flush=True)
    finally:
        shutil.rmtree(out, ignore_errors=True)


def make_model(a, dt, dev):
    if a.model == "schnet":
        return models.SchNet(DS(), dim1=a.dim, dim2=a.dim, dim3=a.dim, gc_count=3, post_fc_count=1, compute_dtype=dt).to(dev).eval()
    if a.model in ("megnet", "mpnn"):
        cls = models.MEGNet if a.model == "megnet" else models.MPNN
        return cls(DS(), dim1=a.dim, dim2=a.dim, dim3=a.dim, gc_count=3, post_fc_count=1, compute_dtype=dt).to(dev).eval()
    return models.CGCNN(DS(), dim1=a.dim, dim2=a.dim, gc_count=4, post_fc_count=1, compute_dtype=dt).to(dev).eval()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--model", choices=("cgcnn", "schnet", "megnet", "mpnn"), default="cgcnn")
    ap.add_argument("--kernel", action="store_true", help="time csrc/linear_de.hip alone against dx + mdl_rbf_expand_bwd")
    ap.add_argument("--stress", action="store_true", help="energy_forces_stress against energy_and_forces, and the strain reduction alone")
    ap.add_argument("--no-trace", action="store_true", help="--stress: skip the kernel-trace child run")
    ap.add_argument("--edges", type=int, default=2600000)
    ap.add_argument("--widths", default="64,100")
    ap.add_argument("--graphs", type=int, default=8192)
    ap.add_argument("--dim", type=int, default=64)
    ap.add_argument("--dtypes", default="fp32,bf16")
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args()
    if a.kernel:
        if a.repeats == 5:
            a.repeats = 20
        return kernel_bench(a)
    if a.stress:
        return stress_bench(a)
    dev = torch.device("cuda")
    packed = pg.pack_structures(structures(a.graphs, a.seed))
    for dt in a.dtypes.split(","):
        torch.manual_seed(a.seed)
        model = make_model(a, dt, dev)
        run = lambda fused: forces.energy_and_forces(model, packed, (0.0, 8.0), fused=fused)
        run(True), run(False)                                                  # warm-up (code objects, allocator)
        (t_f, t_g), ((_, f_f, _), (_, f_g, _)) = timed([lambda: run(True), lambda: run(False)], a.repeats)
        print(json.dumps({"model": a.model, "dtype": dt, "graphs": a.graphs, "atoms": int(packed["node_ptr"][-1]), "dim": a.dim,
                          "fused_ms": round(t_f, 3), "general_ms": round(t_g, 3),
                          "max_abs_diff_rel": float((f_f - f_g).abs().max() / f_f.abs().max())}), flush=True)


if __name__ == "__main__":
    main()
