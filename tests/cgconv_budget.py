"""Per-row error budget of the bf16 CGConv layer against an fp64 reference (helper module of test_cgconv_budget_host.py and
test_gpu_cgconv_budget.py; no test lives here).

The parity tests of the layer bound the largest element error by 3e-2 of the largest element of the whole tensor.  That is
about ten times what the bf16 arithmetic needs, and wide enough for one dropped edge or a degree that is off by one to pass.
Here the yardstick is a ROUNDING MODEL: the layer's arithmetic in plain fp32 torch on the CPU, rounded to bf16 exactly where
the bf16 kernels round.  Its distance from an fp64 run of the oracle is the error the design itself makes; a kernel is allowed
ALLOWED[tensor] times that, per row (row_ratio), and a structural bug in one row stands 20-40x over it (MUTATIONS).
"""
import functools

import torch

from oracle import ops as oops

TENSORS = ("out", "dx", "dW_f", "db_f", "dW_s", "db_s", "de")

LOG2E = float(torch.tensor(1.4426950408889634, dtype=torch.float32))     # Gate<true>::W_SCALE (mdl_common.h:136)
LN2 = float(torch.tensor(0.6931471805599453, dtype=torch.float32))       # Gate<true>::M_SCALE (mdl_common.h:137)

# Permitted row_ratio per tensor: twice the largest value measured on the MI355X over every case of
# test_gpu_cgconv_budget.py, rounded up to one decimal, never below 2 and never above 5.  The factor 2 covers what kernel and
# model draw differently: summation order, the hardware exp2 / log2 / rcp of the fast gate, r_src rounded once per window flush
# or once per packed bf16 atomic against once in the model.
# Measured on the MI355X: row_ratio of every case of test_gpu_cgconv_budget.py against the rounding model.  The backward sums
# with atomics, so dx and dW move in the second decimal from run to run; the rows are one run, `largest` is over two.
#   case                   dispatch       ratios
#   static64               per_wave       out 1.00  dx 1.33  dW_f 1.38  db_f 1.00  dW_s 1.28  db_s 1.00
#   static64               edge_lane      out 1.00  dx 1.49  dW_f 1.56  db_f 0.83  dW_s 1.20  db_s 0.82
#   static64               deterministic  out 1.00  dx 1.37  dW_f 1.32  db_f 1.00  dW_s 1.29  db_s 1.00
#   static64               rsrc16_off     out 1.00  dx 1.22  dW_f 1.01  db_f 1.00  dW_s 1.04  db_s 1.00
#   far_sources            per_wave       out 1.00  dx 1.87  dW_f 1.25  db_f 1.00  dW_s 1.32  db_s 1.00
#   far_sources            edge_lane      out 1.00  dx 1.70  dW_f 1.48  db_f 0.74  dW_s 1.31  db_s 0.62
#   partial_group                         out 1.00  dx 1.30  dW_f 1.59  db_f 1.00  dW_s 1.48  db_s 1.00
#   single_node                           out 1.00  dx 1.00  dW_f 1.00  db_f 1.00  dW_s 1.00  db_s 1.00
#   static32                              out 1.00  dx 1.26  dW_f 1.28  db_f 1.00  dW_s 1.40  db_s 1.00
#   wide128                               out 1.00  dx 1.23  dW_f 1.44  db_f 1.00  dW_s 1.55  db_s 1.00
#   wide100                pad128         out 1.00  dx 1.29  dW_f 1.35  db_f 1.00  dW_s 1.31  db_s 1.00
#   wide100                no_pad128      out 1.00  dx 1.10  dW_f 1.05  db_f 1.00  dW_s 1.03  db_s 1.00
#   bpack_64_64                           out 1.00  dx 1.18  dW_f 1.02  db_f 1.00  dW_s 1.02  db_s 1.00
#   bpack_64_48_no_bias                   out 1.00  dx 1.09  dW_f 1.04  dW_s 1.03
#   bpack_32_16                           out 1.00  dx 1.42  dW_f 1.01  db_f 1.00  dW_s 1.01  db_s 1.00
#   generic_20_7                          out 1.00  dx 1.05  dW_f 1.04  db_f 1.00  dW_s 1.02  db_s 1.00
#   generic_30_7                          out 1.00  dx 1.15  dW_f 1.07  db_f 1.00  dW_s 1.02  db_s 1.00
#   generic_64_41                         out 1.00  dx 1.04  dW_f 1.03  db_f 1.00  dW_s 1.01  db_s 1.00
#   sparse                                out 1.00  dx 1.31  dW_f 1.10  db_f 1.00  dW_s 1.06  db_s 1.00
#   sum                                   out 1.00  dx 1.35  dW_f 1.23  db_f 1.00  dW_s 1.24  db_s 1.00
#   unsorted                              out 1.00  dx 1.53  dW_f 1.25  db_f 1.00  dW_s 1.37  db_s 1.00
#   de_static64                           out 1.00  dx 1.44  dW_f 1.61  db_f 1.00  dW_s 1.32  db_s 1.00  de 1.04
#   de_bpack_64_64                        out 1.00  dx 1.09  dW_f 1.03  db_f 1.00  dW_s 1.03  db_s 1.00  de 1.02
# largest: out 1.00, dx 1.87, dW_f 1.63, db_f 1.00, dW_s 1.55, db_s 1.00, de 1.04
ALLOWED = {"out": 2.0, "dx": 3.8, "dW_f": 3.3, "db_f": 2.0, "dW_s": 3.1, "db_s": 2.0, "de": 2.1}


def bfr(t):
    """round to bf16 (nearest even), keep fp32 storage"""
    return t.to(torch.bfloat16).to(torch.float32)


def _rup(a, b):
    return (a + b - 1) // b * b


def node_path(C):
    """Which node-level half of the backward ops._CGConvFn._backward_main runs in bf16 (ops.py: `node_hip`, the `Cp == 128` branch,
    the library-GEMM branch): it decides where dx and the node columns of dW are rounded."""
    if C in (32, 64):
        return "k3c"
    if _rup(C, 32) == 128 and C % 2 == 0:
        return "wide"
    return "generic"


# ---------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------
SPECIAL_DEGREES = (13, 32, 33, 64, 65, 100)       # the probe, one tile, one tile + 1, two tiles, two tiles + 1, four tiles
PROBE_DEGREE = 13


def budget_graph(n, seed=0, window=40, max_in=20, sort=True):
    """Seeded edge list [2, E] (source, target) with self loops, target-sorted unless sort=False.  For n >= 9: node 0 and node
    n - 1 are isolated; six nodes spread over the rest have in-degree exactly 13 (the probe), 32, 33, 64, 65 and 100 (the edge
    tile of the kernels is 32 slots); every other node draws 1..max_in sources within +-window plus its self loop (sources
    repeat, like in tests/test_gpu_kernels.rand_graph).  Smaller n (the single-node case): every node gets 5 in-edges, no
    specials.  Returns (edge_index, probe) with probe = the degree-13 node or None."""
    g = torch.Generator().manual_seed(1000 + seed)
    src, tgt = [], []
    special = {}
    if n >= 9:
        inner = n - 2
        for k, deg in enumerate(SPECIAL_DEGREES):
            special[1 + (2 * k + 1) * inner // (2 * len(SPECIAL_DEGREES))] = deg
        assert len(special) == len(SPECIAL_DEGREES)
    for i in range(n):
        if n >= 9 and i in (0, n - 1):
            continue
        lo, hi = max(0, i - window), min(n, i + window)
        k = special[i] - 1 if i in special else (int(torch.randint(1, max_in + 1, (1,), generator=g)) if n >= 9 else 4)
        s = torch.randint(lo, hi, (k,), generator=g).tolist() + [i]
        src += s
        tgt += [i] * len(s)
    ei = torch.tensor([src, tgt], dtype=torch.int64)
    if not sort:
        ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    probe = next((i for i, d in special.items() if d == PROBE_DEGREE), None)
    return ei, probe


def sparse_graph(n, nodes_with_edges, seed=0, max_in=14):
    """Target-sorted graph in which most nodes are isolated: `nodes_with_edges` random nodes draw 1..max_in sources from anywhere
    plus a self loop.  N >~ E: the shape at which the backward takes 32-node groups from a counter (cg_launch: `p.ctr`, g_full)."""
    g = torch.Generator().manual_seed(2000 + seed)
    who = torch.sort(torch.randperm(n, generator=g)[:nodes_with_edges]).values.tolist()
    src, tgt = [], []
    for i in who:
        k = int(torch.randint(1, max_in + 1, (1,), generator=g))
        s = torch.randint(0, n, (k,), generator=g).tolist() + [i]
        src += s
        tgt += [i] * len(s)
    return torch.tensor([src, tgt], dtype=torch.int64)


def layer_inputs(ei, n, C, G, seed, bias=True):
    """x, edge_attr, W_f, b_f, W_s, b_s, grad_out as fp32 tensors that are exact in bf16 (biases stay fp32: the layer keeps them
    so), with the weight scaling of tests/test_gpu_kernels._cgconv_case."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = bfr(rnd(n, C))
    ea = bfr(torch.rand(ei.shape[1], G, generator=g))
    k = 3.0 / (2 * C + G) ** 0.5
    wf, ws = bfr(rnd(C, 2 * C + G) * k), bfr(rnd(C, 2 * C + G) * k)
    bf, bs = rnd(C) * 0.1, rnd(C) * 0.1
    gout = bfr(rnd(n, C))
    if not bias:
        bf = bs = None
    return dict(x=x, ei=ei, ea=ea, wf=wf, bf=bf, ws=ws, bs=bs, gout=gout)


# ---------------------------------------------------------------------------------------------
# fp64 reference
# ---------------------------------------------------------------------------------------------
def reference64(x, ei, ea, wf, bf, ws, bs, gout, aggr="mean", need_de=False):
    """oracle.ops.cgconv in float64 on the inputs as stored (already rounded to bf16), loss = sum(out * gout):
    dict of out, dx, dW_f, db_f, dW_s, db_s (None without a bias) and de when asked."""
    d = lambda t: None if t is None else t.double().clone().requires_grad_(True)
    x64, e64, wf64, bf64, ws64, bs64 = d(x), d(ea), d(wf), d(bf), d(ws), d(bs)
    out = oops.cgconv(x64, ei, e64, wf64, bf64, ws64, bs64, aggr)
    (out * gout.double()).sum().backward()
    g = lambda t: None if t is None else t.grad
    r = dict(out=out.detach(), dx=x64.grad, dW_f=wf64.grad, db_f=g(bf64), dW_s=ws64.grad, db_s=g(bs64))
    if need_de:
        r["de"] = e64.grad
    return r


# ---------------------------------------------------------------------------------------------
# rounding model
# ---------------------------------------------------------------------------------------------
def rounding_model(x, ei, ea, wf, bf, ws, bs, gout, aggr="mean", need_de=False, mutation=None, probe=None):
    """The bf16 layer in plain fp32 torch on the CPU, rounded to bf16 where the bf16 kernels round and nowhere else.  It follows
    the arithmetic, not the tiling: no groups, tiles, waves or windows.  Rounding points (paths below matdeeplearn_amd/):

    forward
      F1  packed weights bf16(W * log2 e): the scale is applied before the rounding       csrc/cgconv.hip:122 (cgconv_pack_body)
      F2  bias: G % 16 != 0 -> a K column of the packed weights, bf16(b * log2 e)           csrc/cgconv.hip:97,122
                G % 16 == 0 -> fp32 b * log2 e, seeds the accumulators                      csrc/cgconv.hip:127, csrc/cgconv_fwd.inc:36,242
      --  pre = z W^T: exact bf16 products, fp32 sums (MFMA); base-2 gate in fp32           csrc/mdl_common.h:151-156
      F3  message sigmoid * softplus / ln 2 rounded to bf16 as the operand of the one-hot
          aggregation MFMA, fp32 sums                                                       csrc/cgconv_tiles.inc:520 (seg_reduce_mma)
      F4  out = x + sum * ln 2 * (1 / deg) rounded on store                                 csrc/cgconv_fwd.inc:331-334,460-465
    backward edge pass
      B1  grad_out * (1 / deg) rounded to bf16 as the operand of the one-hot expansion      csrc/cgconv_bwd.inc:127-129
          (the edge-per-lane kernel scales in fp32 instead, csrc/cgconv_ep2.inc:217: it rounds less than the model here)
      B2  dpre rounded to bf16 as an MFMA operand                                           csrc/cgconv_bwd.inc:282 (DFrags::pack), csrc/cgconv_ep2.inc:226
      B3  r_tgt (sums of B2 by target, fp32) stored in the compute dtype                    csrc/cgconv_bwd.inc:414-415
      --  db = column sums of the UNROUNDED r_tgt, dW[:, 2C:] = dpre^T e: fp32              csrc/cgconv_bwd.inc:408,332
      B4  r_src (sums of B2 by source) in bf16: with rsrc16 once per window flush / packed
          atomic, without it as the node kernel's MFMA operand; the model rounds ONCE       csrc/cgconv_bwd.inc:389, csrc/cgconv_node.hip:128, ops.py:882,899
    backward node part
      B5  Wn: the UNSCALED bf16 weights                                                     csrc/cgconv.hip:86 (wn_t)
      B6  dx = g + [r_tgt | r_src] Wn rounded on store; the wide path (C = 100 / 128)
          rounds after the r_tgt product and again after the r_src product                  csrc/cgconv_node.hip:176, ops.py:887-888,900
      B7  node columns of dW = [r_tgt | r_src]^T x in fp32; the library-GEMM path of the
          other widths returns them in bf16                                                 csrc/cgconv_node.hip:205, ops.py:901
    edge-feature gradient
      D1  dpre from the UNROUNDED grad_out / deg, rounded to bf16 as an MFMA operand        csrc/cgconv_de.hip:127,138
      D2  de = (dpre We) / log2 e with the packed (scaled) weights F1, rounded on store     csrc/cgconv_de.hip:149,168

    mutation: a key of MUTATIONS (a kernel bug in miniature, applied around `probe`), or None."""
    n, C = x.shape
    E, G = ea.shape
    row, col = ei[0], ei[1]
    mut = MUTATIONS[mutation](ei, n, probe) if mutation else {}
    f32 = torch.float32
    one = torch.ones(E, dtype=f32)
    deg = torch.zeros(n, dtype=f32).index_add_(0, col, one).clamp(min=1)
    if "deg" in mut:
        deg = deg.clone()
        deg[mut["deg"][0]] += mut["deg"][1]
    invd = (1.0 / deg) if aggr == "mean" else torch.ones(n, dtype=f32)
    keep_f = mut.get("keep_fwd", one)                       # 0 for an edge the forward sum misses
    keep_b = mut.get("keep_bwd", one)
    row_x = mut.get("row_x", row)                           # where x_src is read from

    bias_col = G % 16 != 0
    wpf, wps = bfr(wf * LOG2E), bfr(ws * LOG2E)                                                    # F1
    pb = lambda b: torch.zeros(C, dtype=f32) if b is None else (bfr(b * LOG2E) if bias_col else b * LOG2E)   # F2
    bpf, bps = pb(bf), pb(bs)
    z = torch.cat([x.index_select(0, col), x.index_select(0, row_x), ea], dim=1)
    tf, ts = z @ wpf.t() + bpf, z @ wps.t() + bps           # base-2 pre-activations
    sf = 1.0 / (1.0 + torch.exp2(-tf))
    sp_u = torch.clamp(ts, min=0) + torch.log2(1.0 + torch.exp2(-ts.abs()))
    ss = 1.0 / (1.0 + torch.exp2(-ts))
    m = bfr(sf * sp_u) * keep_f.view(-1, 1)                                                         # F3
    acc = torch.zeros(n, C, dtype=f32).index_add_(0, col, m)
    out = bfr(x + (acc * LN2) * invd.view(-1, 1))                                                   # F4

    def dpre(gd):
        t = gd.index_select(0, col) * sf
        return bfr((t * LN2) * (1.0 - sf) * sp_u) * keep_b.view(-1, 1), bfr(t * ss) * keep_b.view(-1, 1)   # B2 / D1
    dpf, dps = dpre(bfr(gout * invd.view(-1, 1)))                                                   # B1
    by = lambda idx, v: torch.zeros(n, C, dtype=f32).index_add_(0, idx, v)
    rtf32, rts32 = by(col, dpf), by(col, dps)
    db_f, db_s = rtf32.sum(0), rts32.sum(0)
    rtf, rts = bfr(rtf32), bfr(rts32)                                                               # B3
    rsf, rss = bfr(by(row_x, dpf)), bfr(by(row_x, dps))                                             # B4
    path = node_path(C)
    wn = [bfr(w[:, a:a + C]) for a in (0, C) for w in (wf, ws)]      # f_tgt, s_tgt, f_src, s_src      B5
    if path == "wide":
        dx = bfr(bfr(gout + rtf @ wn[0] + rts @ wn[1]) + rsf @ wn[2] + rss @ wn[3])                # B6
    else:
        dx = bfr(gout + rtf @ wn[0] + rts @ wn[1] + rsf @ wn[2] + rss @ wn[3])                     # B6
    nd = (lambda t: bfr(t)) if path == "generic" else (lambda t: t)                                 # B7
    dW_f = torch.cat([nd(rtf.t() @ x), nd(rsf.t() @ x), dpf.t() @ ea], dim=1)
    dW_s = torch.cat([nd(rts.t() @ x), nd(rss.t() @ x), dps.t() @ ea], dim=1)
    if "zero" in mut:                                       # (node, channel) a store misses
        i, c = mut["zero"]
        out[i, c] = 0.0
        dx[i, c] = 0.0
    r = dict(out=out, dx=dx, dW_f=dW_f, db_f=db_f if bf is not None else None, dW_s=dW_s, db_s=db_s if bs is not None else None)
    if need_de:
        ef, es = dpre(gout * invd.view(-1, 1))                                                      # D1
        r["de"] = bfr((ef @ wpf[:, 2 * C:] + es @ wps[:, 2 * C:]) * (1.0 / LOG2E))                  # D2
    return r


# ---------------------------------------------------------------------------------------------
# mutations: edits of the MODEL, each a kernel bug in miniature.  ei -> what rounding_model changes.
# ---------------------------------------------------------------------------------------------
def _csr_order(ei):
    return torch.sort(ei[1], stable=True).indices


def _probe_edge(ei, probe, which=5):
    """the `which`-th in-edge (CSR order) of the probe node whose source is not the probe itself"""
    order = _csr_order(ei)
    own = [int(e) for e in order if int(ei[1, e]) == probe and int(ei[0, e]) != probe]
    return own[min(which, len(own) - 1)]


def _keep_without(ei, edges):
    k = torch.ones(ei.shape[1], dtype=torch.float32)
    k[edges] = 0.0
    return k


def _mut_drop_fwd(ei, n, probe):
    return {"keep_fwd": _keep_without(ei, [_probe_edge(ei, probe)])}


def _mut_drop_bwd(ei, n, probe):
    return {"keep_bwd": _keep_without(ei, [_probe_edge(ei, probe)])}


def _mut_degree(ei, n, probe):
    return {"deg": (probe, 1.0)}


def _mut_tile(ei, n, probe):
    order = _csr_order(ei)
    pos = int((ei[1, order] == probe).nonzero()[0])
    t0 = pos // 32 * 32
    k = _keep_without(ei, order[t0:t0 + 32])
    return {"keep_fwd": k, "keep_bwd": k}


def _mut_last_channel(ei, n, probe):
    return {"zero": (n - 1, -1)}


def _mut_neighbour_source(ei, n, probe):
    e = _probe_edge(ei, probe)
    row_x = ei[0].clone()
    row_x[e] = row_x[e] + 1 if int(row_x[e]) + 1 < n else row_x[e] - 1
    return {"row_x": row_x}


MUTATIONS = {
    "edge_dropped_forward": _mut_drop_fwd,            # one edge of the probe node left out of the forward sum
    "edge_dropped_backward": _mut_drop_bwd,           # the same edge left out of the backward
    "degree_off_by_one": _mut_degree,                 # the probe node's mean divisor is deg + 1
    "tile_dropped": _mut_tile,                        # the 32-slot edge tile that holds the probe's first edge left out
    "last_channel_not_stored": _mut_last_channel,     # last channel of the last node's row left at zero
    "source_from_neighbour": _mut_neighbour_source,   # x_src of one edge of the probe read from the next node
}


# ---------------------------------------------------------------------------------------------
# the measure
# ---------------------------------------------------------------------------------------------
def _rows(t):
    t = t.detach().double().cpu()
    return t.reshape(1, -1) if t.dim() < 2 else t.reshape(t.shape[0], -1)


def row_rms(a, ref64):
    return (_rows(a) - _rows(ref64)).pow(2).mean(dim=1).sqrt()


def row_ratio(got, model, ref64):
    """Largest over rows of  rms_row(got - ref64) / max(rms_row(model - ref64), median over rows of rms_row(model - ref64)).
    Rows: output nodes for out / dx, output channels for dW, edges for de; a 1-D tensor is one row.  The floor keeps rows
    where the model happens to be exact (an isolated node: out = x) from dividing by zero."""
    e_got, e_mod = row_rms(got, ref64), row_rms(model, ref64)
    den = torch.clamp(e_mod, min=float(e_mod.median()))
    # (a graph of mostly isolated nodes has a zero median: a row that model and kernel both get exactly right counts 0, a row
    # that only the model gets exactly right counts infinity)
    return float(torch.where(e_got == 0, torch.zeros_like(e_got), e_got / den).max())


def ratios(got, model, ref64):
    """{tensor: row_ratio} over the tensors present in ref64 (a missing bias has none)"""
    return {k: row_ratio(got[k], model[k], ref64[k]) for k in TENSORS if ref64.get(k) is not None}


def fmt(r):
    return "  ".join("%s %.2f" % (k, v) for k, v in r.items())


# ---------------------------------------------------------------------------------------------
# the cases of test_gpu_cgconv_budget.py: inputs, fp64 reference and model, computed once per process and never modified
# ---------------------------------------------------------------------------------------------
# name -> (n, C, G, graph keywords, aggr, bias, need_de)
CASES = {
    "static64": (200, 64, 50, {}, "mean", True, False),
    "far_sources": (700, 64, 50, {"window": 400}, "mean", True, False),
    "partial_group": (33, 64, 50, {}, "mean", True, False),
    "single_node": (1, 64, 50, {}, "mean", True, False),
    "static32": (100, 32, 50, {}, "mean", True, False),
    "wide128": (65, 128, 50, {}, "mean", True, False),
    "wide100": (130, 100, 50, {}, "mean", True, False),
    "bpack_64_64": (200, 64, 64, {}, "mean", True, False),
    "bpack_64_48_no_bias": (200, 64, 48, {}, "mean", False, False),
    "bpack_32_16": (100, 32, 16, {}, "mean", True, False),
    "generic_20_7": (100, 20, 7, {}, "mean", True, False),
    "generic_30_7": (100, 30, 7, {}, "mean", True, False),
    "generic_64_41": (100, 64, 41, {}, "mean", True, False),
    "sparse": (2000, 64, 50, {"sparse": 200}, "mean", True, False),
    "sum": (200, 64, 50, {}, "add", True, False),
    "unsorted": (200, 64, 50, {"sort": False}, "mean", True, False),
    "de_static64": (200, 64, 50, {}, "mean", True, True),
    "de_bpack_64_64": (200, 64, 64, {}, "mean", True, True),
}


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(inputs, probe, aggr, need_de, ref, model) of a named case; shared, read-only"""
    n, C, G, gkw, aggr, bias, need_de = CASES[name]
    seed = sorted(CASES).index(name)
    if "sparse" in gkw:
        ei, probe = sparse_graph(n, gkw["sparse"], seed), None
    else:
        ei, probe = budget_graph(n, seed=seed, **gkw)
    inp = layer_inputs(ei, n, C, G, seed=100 + seed, bias=bias)
    ref = reference64(aggr=aggr, need_de=need_de, **inp)
    model = rounding_model(aggr=aggr, need_de=need_de, **inp)
    return dict(inputs=inp, probe=probe, aggr=aggr, need_de=need_de, ref=ref, model=model, n=n, C=C, G=G,
                sorted="sort" not in gkw)


def mutated(name, mutation):
    c = case(name)
    return rounding_model(aggr=c["aggr"], need_de=c["need_de"], mutation=mutation, probe=c["probe"], **c["inputs"])
