"""Per-row error budget of the bf16 NNConv kernels against an fp64 reference (helper module of test_nnconv_budget_host.py and
test_gpu_nnconv_budget.py; no test lives here).  It follows tests/cgconv_budget.py and tests/cfconv_budget.py: the yardstick is a
ROUNDING MODEL, the same arithmetic in plain fp32 torch on the CPU, rounded to bf16 exactly where the kernels round.  Its distance
from an fp64 run is the error the design itself makes; a kernel is allowed ALLOWED[tensor] times that, per row (row_ratio), and a
structural bug in one row stands far over it (MUTATIONS, LAYER_MUTATIONS).

Two levels:
  op     K7 alone (csrc/nnconv.hip) through the C ABI, on every route of its dispatch (k7_route):
             m[e] = Y[src_e] (Co x D3) . h[e]      dh[e] = Y[src_e]^T . dm[e]      dY[j] = sum_{e out of j} dm[e] (x) h[e]
  layer  nn.NNConv in bf16, forward and backward, against oracle.ops.NNConv in fp64
"""
import functools

import torch

from cgconv_budget import bfr, budget_graph, fmt, row_ratio, row_rms  # noqa: F401  (re-exported for the tests)
from cgconv_budget import PROBE_DEGREE, SPECIAL_DEGREES
from cfconv_budget import HUB_OUT_DEGREES, cf_graph
from oracle import ops as oops

OP_TENSORS = ("m", "dh", "dY")
# rows: edges (m, dh), (node, output unit) pairs for dY — [n * Co, D3]: one wrong element is not diluted over a 10^4-element row
LAYER_TENSORS = ("out", "dx", "dW_nn0", "db_nn0", "dW_nn2", "db_nn2", "dW_root", "db")
# rows: nodes (out, dx), output units (the weights), one row (the biases)
TENSORS = OP_TENSORS + LAYER_TENSORS

# Permitted row_ratio per tensor: twice the largest value measured on the MI355X over every case of test_gpu_nnconv_budget.py
# against the rounding model, rounded up to one decimal, never below 2 and never above 5.  The factor 2 covers what kernel and
# model draw differently: the summation order (MFMA against fp32 torch, 32-edge chunks, atomics in the weight-gradient GEMMs).
# Measured on the MI355X: row_ratio of every case of test_gpu_nnconv_budget.py against the rounding model (three decimals here;
# `largest` from four).  dW_root = g^T x has exact bf16 operands on both sides: its model error IS fp32 summation noise, and
# the TN GEMM sums with atomics, so it alone moves from run to run (0.86 .. 1.05); the rows are one run, `largest` is over two.
#   case               route                          ratios
#   w100               mfma fwd flat bwd flat <5>     m 1.000  dh 1.000  dY 1.000
#   at_small_limit     mfma fwd flat bwd flat <5>     m 1.000  dh 1.000  dY 1.000
#   over_small_limit   mfma fwd flat bwd flat <7>     m 1.000  dh 1.000  dY 1.000
#   full_budget        mfma fwd flat bwd flat <7>     m 1.000  dh 1.000  dY 1.000
#   too_big            mfma fwd dense bwd dense <7>   m 1.000  dh 1.000  dY 1.000
#   odd_bytes          mfma fwd dense bwd dense <7>   m 1.000  dh 1.000  dY 1.000
#   overrun30          mfma fwd flat bwd flat <5>     m 1.000  dh 1.000  dY 1.000
#   smallest_flat      mfma fwd flat bwd flat <5>     m 1.000  dh 1.000  dY 1.000
#   d3_two             mfma fwd dense bwd dense <7>   m 1.000  dh 1.000  dY 1.000
#   y_misaligned       mfma fwd dense bwd dense <7>   m 1.000  dh 1.000  dY 1.000
#   dy_misaligned      mfma fwd flat bwd dense <7>    m 1.000  dh 1.000  dY 1.000
#   by_source_null     mfma fwd flat bwd flat <5>     m 1.000  dh 1.000  dY 1.000
#   scalar_odd         scalar                         m 1.000  dh 1.000  dY 1.000
#   scalar_wide_co     scalar                         m 1.000  dh 1.000  dY 1.000
#   scalar_wide_d3     scalar                         m 1.000  dh 1.000  dY 1.000
#   layer_small        library x @ w                  out 1.000  dx 1.000  dW_nn0 1.000  db_nn0 1.000  dW_nn2 1.005  db_nn2 1.000  dW_root 1.038  db 1.000
#   layer_wide_24      linear_wide kp 64, 4 blocks    out 1.000  dx 1.000  dW_nn0 1.003  db_nn0 1.000  dW_nn2 1.003  db_nn2 1.000  dW_root 0.922  db 1.000
#   layer_wide_100     linear_wide kp 128, 53 blocks  out 1.012  dx 1.000  dW_nn0 1.002  db_nn0 1.000  dW_nn2 1.004  db_nn2 1.000  dW_root 1.054  db 1.000
#   layer_add          library x @ w                  out 1.008  dx 1.000  dW_nn0 1.000  db_nn0 1.000  dW_nn2 1.001  db_nn2 1.000  dW_root 1.049  db 1.000
# largest: m 1.0000, dh 1.0000, dY 1.0000, out 1.0115 (layer_wide_100), dx 1.0000, dW_nn0 1.0034 (layer_wide_24), db_nn0 1.0001,
# dW_nn2 1.0054 (layer_small), db_nn2 1.0000, dW_root 1.0544 (layer_wide_100), db 1.0000.
# No ratio came near 2.5: no rounding point is missing from the models, and no kernel bug was found.
ALLOWED = {"m": 2.0, "dh": 2.0, "dY": 2.0, "out": 2.1, "dx": 2.0, "dW_nn0": 2.1, "db_nn0": 2.1, "dW_nn2": 2.1, "db_nn2": 2.0,
           "dW_root": 2.2, "db": 2.0}

PAD = 77                                         # edge rows of m / dh that belong to no by-source segment
GUARD = 256                                      # bytes behind every output in the arena of the GPU test


# ---------------------------------------------------------------------------------------------
# graphs
# ---------------------------------------------------------------------------------------------
def nn_graph(n, seed=0, sort=True, by_source=False, **kw):
    """cf_graph (in-degrees 13 / 32 / 33 / 64 / 65 / 100, hub sources of out-degree exactly 100 and 33) with THREE NODES OF
    OUT-DEGREE 0 on top — node 0, node n - 1 and one inner node that is neither a hub nor a special-degree node: their out-edges
    are handed to the nearest following (for node n - 1: preceding) source that is neither a hub nor one of the three.  Only
    sources change, so every in-degree is budget_graph's, and no hub gains or loses an edge.  K7 runs one workgroup per SOURCE:
    these are the nodes of its `b == e` branch (no message; dY_j = 0).
    by_source: the edge list is (stably) sorted by source, the order in which K7 takes `eid_s = NULL`.
    Returns (edge_index, probe, hub33, hub100, zeros) — the degree-13 node, the two hubs, the three nodes without out-edges."""
    assert n >= 30
    ei, probe, hub33 = cf_graph(n, seed=seed, sort=sort, **kw)
    src, tgt = ei[0].clone(), ei[1]
    indeg = torch.bincount(tgt, minlength=n)
    plain = [i for i in range(1, n - 1) if int(indeg[i]) not in SPECIAL_DEGREES]
    hubs = (plain[len(plain) // 3], plain[2 * len(plain) // 3])          # cf_graph's choice, restated
    assert hubs[1] == hub33
    inner = next(i for i in plain[len(plain) // 2:] if i not in hubs)
    zeros = (0, inner, n - 1)
    for z in zeros:
        step = -1 if z == n - 1 else 1
        s = z + step
        while s in hubs or s in zeros:
            s += step
        src[src == z] = s
    ei = torch.stack([src, tgt])
    if by_source:
        ei = ei[:, torch.sort(ei[0], stable=True).indices]
    return ei, probe, hubs[1], hubs[0], zeros


def by_source_csr(ei, n):
    """(rowptr_s [n + 1] int32, eid_s [E] int32): the by-source CSR of EdgeCSR.transposed() — eid_s is the stable argsort of the
    sources, the caller's edge id per slot"""
    eid = torch.sort(ei[0], stable=True).indices
    rowptr = torch.zeros(n + 1, dtype=torch.int64)
    rowptr[1:] = torch.cumsum(torch.bincount(ei[0], minlength=n), 0)
    return rowptr.to(torch.int32), eid.to(torch.int32)


# ---------------------------------------------------------------------------------------------
# the dispatch of K7, restated: the kernel choice is made in C and is not observable from Python
# ---------------------------------------------------------------------------------------------
K7_CHUNK_BUDGET = 256 * 7 * 8                    # elements of Y_j that 256 threads x 7 chunks x 16 bytes hold
K7_SMALL_BUDGET = 256 * 5 * 8                    # ... x K7_BWD_SMALLC = 5 chunks


def k7_route(Co, D3, y_mod16=0, dy_mod16=0):
    """(kind, fwd_flat, bwd_flat, bwd_maxc) of a bf16 call of mdl_nnconv_msg_fwd / _bwd with Y at y_mod16 and dY at dy_mod16
    bytes past a 16-byte boundary (h, dm, m and dh dword-aligned), read off matdeeplearn_amd/csrc/nnconv.hip:
      kind      "mfma" if nm_ok (lines 426-429: both sizes even and in [2, 128], dword-aligned pointers) else "scalar"
      fwd_flat  the flat staging of Y_j in the forward (line 453: D3 >= 4, Co * D3 * 2 bytes a multiple of 16, Y on a 16-byte
                boundary, Co * D3 within the budget of seven chunks per thread)
      bwd_flat  the same in the backward, which also asks dY onto a 16-byte boundary (lines 486-487)
      bwd_maxc  the instantiation of nnconv_msg_bwd_mfma_kernel: 5 for a flat block of at most 10240 elements, else 7 (lines
                491-500); 0 for the scalar kernels"""
    assert y_mod16 % 4 == 0 and dy_mod16 % 4 == 0, "the mirror covers dword-aligned pointers"
    if not (2 <= Co <= 128 and 2 <= D3 <= 128 and Co % 2 == 0 and D3 % 2 == 0):
        return ("scalar", False, False, 0)
    shape_flat = D3 >= 4 and (Co * D3 * 2) % 16 == 0 and Co * D3 <= K7_CHUNK_BUDGET
    fwd_flat = shape_flat and y_mod16 == 0
    bwd_flat = fwd_flat and dy_mod16 == 0
    return ("mfma", fwd_flat, bwd_flat, 5 if bwd_flat and Co * D3 <= K7_SMALL_BUDGET else 7)


# ---------------------------------------------------------------------------------------------
# op level: inputs, fp64 reference, rounding model
# ---------------------------------------------------------------------------------------------
def k7_inputs(ei, n, Co, D3, seed):
    """Y [n, Co * D3] ~ N(0, 1 / D3), h [E, D3] = relu(randn) (the real h is post-ReLU: exact zeros), dm [E, Co]: fp32 tensors
    that are exact in bf16"""
    g = torch.Generator().manual_seed(seed)
    E = ei.shape[1]
    Y = bfr(torch.randn(n, Co * D3, generator=g) / D3 ** 0.5)
    h = bfr(torch.relu(torch.randn(E, D3, generator=g)))
    dm = bfr(torch.randn(E, Co, generator=g))
    return dict(Y=Y, h=h, dm=dm, ei=ei, n=n, Co=Co, D3=D3)


def _segments(src, n):
    order = torch.sort(src, stable=True).indices
    ptr = [0] + torch.cumsum(torch.bincount(src, minlength=n), 0).tolist()
    return order, ptr


def k7_contract(Y, h, dm, ei, n, Co, D3, dtype, mut=None):
    """the three contractions in `dtype`, source node by source node (no E x Co x D3 tensor); mut: what a mutation changes"""
    mut = mut or {}
    E = ei.shape[1]
    src = ei[0]
    Yv = Y.to(dtype).view(n, Co, D3)
    h, dm = h.to(dtype), dm.to(dtype)
    h_m, src_m, dm_h = mut.get("h_m", h).to(dtype), mut.get("src_m", src), mut.get("dm_dh", dm).to(dtype)
    keep = mut.get("keep_dY", torch.ones(E)).to(dtype).view(-1, 1)
    m, dh = torch.zeros(E, Co, dtype=dtype), torch.zeros(E, D3, dtype=dtype)
    dY = torch.zeros(n, Co, D3, dtype=dtype)
    order, ptr = _segments(src, n)
    order_m, ptr_m = _segments(src_m, n) if "src_m" in mut else (order, ptr)
    for j in range(n):
        e = order_m[ptr_m[j]:ptr_m[j + 1]]
        if e.numel():
            m[e] = h_m[e] @ Yv[j].t()
        e = order[ptr[j]:ptr[j + 1]]
        if e.numel():
            dh[e] = dm_h[e] @ Yv[j]
            dY[j] = (dm[e] * keep[e]).t() @ h[e]
    return dict(m=m, dh=dh, dY=dY.view(n, Co * D3))


def k7_reference64(Y, h, dm, ei, n, Co, D3):
    return k7_contract(Y, h, dm, ei, n, Co, D3, torch.float64)


def k7_model(Y, h, dm, ei, n, Co, D3, mutation=None, probes=None):
    """K7 in plain fp32 torch, rounded to bf16 where the kernels store and nowhere else (csrc/nnconv.hip): the operands are bf16
    values, so every product is exact in fp32; the sums are fp32 (MFMA accumulators, fmaf chains in the scalar kernels);
      m    f2bf at line 301 (MFMA), Elem<T>::st at line 55 (scalar)
      dh   f2bf at line 372,       Elem<T>::st at line 101
      dY   f2bf at line 396 (written from the accumulators) / 415 (through LDS, the flat form), Elem<T>::st at line 116
    mutation: a key of MUTATIONS (a kernel bug in miniature, applied around `probes` = (hub33, hub100)), or None."""
    mut = MUTATIONS[mutation][0](_Ctx(Y, h, dm, ei, n, Co, D3, probes)) if mutation else {}
    r = {k: bfr(v) for k, v in k7_contract(Y, h, dm, ei, n, Co, D3, torch.float32, mut).items()}
    if "zero_dY" in mut:                            # one element a store misses: the last column of the (node, unit) row in which
        v = r["dY"].view(n * Co, D3)                # that column is largest against the row's RMS
        row = int((v[:, -1].abs() / v.pow(2).mean(1).sqrt().clamp(min=1e-30)).argmax())
        v[row, -1] = 0.0
    return r


class _Ctx:
    def __init__(self, Y, h, dm, ei, n, Co, D3, probes):
        self.Y, self.h, self.dm, self.ei, self.n, self.Co, self.D3 = Y, h, dm, ei, n, Co, D3
        self.hub33, self.hub100 = probes
        self.order, self.ptr = _segments(ei[0], n)
        self.E = ei.shape[1]

    def out_edges(self, j):
        """edge ids of node j's out-edges in by-source slot order (the order in which K7 walks them)"""
        return self.order[self.ptr[j]:self.ptr[j + 1]]

    def keep_without(self, edges):
        k = torch.ones(self.E, dtype=torch.float32)
        k[edges] = 0.0
        return k


def _mut_last_h_col(c):
    h = c.h.clone()
    h[c.out_edges(c.hub33), -1] = 0.0
    return {"h_m": h}


def _mut_y_next_node(c):
    """the 33-hub's out-edge with the largest h row takes Y from node hub + 1"""
    own = c.out_edges(c.hub33)
    e = int(own[int(c.h[own].pow(2).sum(1).argmax())])
    s = c.ei[0].clone()
    s[e] = s[e] + 1
    return {"src_m": s}


def _mut_last_y_row(c):
    dm = c.dm.clone()
    dm[c.out_edges(c.hub33), -1] = 0.0
    return {"dm_dh": dm}


M_, DH_, DY_ = ("m",), ("dh",), ("dY",)
# name -> (edit, the tensor of the ONE kernel output the mutation models)
MUTATIONS = {
    "last_h_column_m": (_mut_last_h_col, M_),                    # the last h column is not read for the 33-hub's edges
    "y_from_next_node_m": (_mut_y_next_node, M_),                # Y is taken from node j + 1 for one edge
    "last_y_row_dh": (_mut_last_y_row, DH_),                     # the last Y row is missing from dh for the 33-hub
    "ragged_edge_dY": (lambda c: {"keep_dY": c.keep_without(c.out_edges(c.hub33)[32:33])}, DY_),   # the 33rd edge of the 33-hub
    "chunk_dropped_dY": (lambda c: {"keep_dY": c.keep_without(c.out_edges(c.hub100)[64:96])}, DY_),  # the third 32-edge chunk
    "one_elem_dY": (lambda c: {"zero_dY": True}, DY_),           # one dY element is not stored
}


def op_rows(name, t, Co, D3):
    return t.reshape(-1, D3) if name == "dY" else t


def op_ratios(got, model, ref64, Co, D3, names=OP_TENSORS):
    return {k: row_ratio(op_rows(k, got[k], Co, D3), op_rows(k, model[k], Co, D3), op_rows(k, ref64[k], Co, D3)) for k in names}


# name -> (Co, D3, the route k7_route must return, keywords: y_off / dy_off in BYTES, by_source)
OP_N = 100
OP_CASES = {
    "w100": (100, 100, ("mfma", True, True, 5), {}),                          # the workload
    "at_small_limit": (128, 80, ("mfma", True, True, 5), {}),                 # 10240: the last shape of bwd <5>
    "over_small_limit": (104, 100, ("mfma", True, True, 7), {}),              # 10400: flat, bwd <7>
    "full_budget": (128, 112, ("mfma", True, True, 7), {}),                   # 14336: all 7 chunks of every thread
    "too_big": (128, 128, ("mfma", False, False, 7), {}),                     # over the chunk budget
    "odd_bytes": (30, 34, ("mfma", False, False, 7), {}),                     # Co * D3 * 2 % 16 != 0, k padded 34 -> 48
    "overrun30": (34, 20, ("mfma", True, True, 5), {}),                       # the forward's last row block runs 30 rows into H
    "smallest_flat": (2, 4, ("mfma", True, True, 5), {}),                     # one 16-byte chunk
    "d3_two": (4, 2, ("mfma", False, False, 7), {}),                          # D3 < 4
    "y_misaligned": (100, 100, ("mfma", False, False, 7), {"y_off": 4}),
    "dy_misaligned": (100, 100, ("mfma", True, False, 7), {"dy_off": 4}),
    "by_source_null": (100, 100, ("mfma", True, True, 5), {"by_source": True}),   # eid_s = NULL
    "scalar_odd": (25, 33, ("scalar", False, False, 0), {}),
    "scalar_wide_co": (130, 100, ("scalar", False, False, 0), {}),            # 13000 > 12288: the second RMAX pass
    "scalar_wide_d3": (24, 130, ("scalar", False, False, 0), {}),
}
# cases whose inputs are drawn from another seed so that every mutation meets the sensitivity condition
# (test_nnconv_budget_host.py holds every case to it)
OP_SEED_SHIFT = {"d3_two": 3}                    # (shifts 0 - 2: both h values of the 33-hub's 33rd edge are zero — dropping it is no bug)


@functools.lru_cache(maxsize=None)
def op_case(name):
    """dict(inputs, probes, zeros, rowptr_s, eid_s, ref, model, route, ...) of a named op-level case; shared, read-only"""
    Co, D3, route, kw = OP_CASES[name]
    seed = sorted(OP_CASES).index(name)
    ei, probe, hub33, hub100, zeros = nn_graph(OP_N, seed=seed, by_source=kw.get("by_source", False))
    inp = k7_inputs(ei, OP_N, Co, D3, seed=200 + seed + 1000 * OP_SEED_SHIFT.get(name, 0))
    rowptr_s, eid_s = by_source_csr(ei, OP_N)
    if kw.get("by_source"):
        assert torch.equal(eid_s, torch.arange(ei.shape[1], dtype=torch.int32))
        eid_s = None
    return dict(inputs=inp, probes=(hub33, hub100), zeros=zeros, rowptr_s=rowptr_s, eid_s=eid_s, ref=k7_reference64(**inp),
                model=k7_model(**inp), route=route, n=OP_N, Co=Co, D3=D3, E=ei.shape[1], y_off=kw.get("y_off", 0),
                dy_off=kw.get("dy_off", 0))


def op_mutated(name, mutation):
    c = op_case(name)
    return k7_model(mutation=mutation, probes=c["probes"], **c["inputs"])


# ---------------------------------------------------------------------------------------------
# layer level: nn.NNConv in bf16
# ---------------------------------------------------------------------------------------------
G = 50                                           # edge features (the Gaussian expansion's width in MPNN)


def layer_inputs(ei, n, Ci, Co, D3, seed):
    """x [n, Ci], edge_attr [E, G] in [0, 1), the weights of nn = Sequential(Linear(G, D3), ReLU, Linear(D3, Ci * Co)) and of the
    root Linear(Ci, Co), grad_out [n, Co] as fp32 tensors that are exact in bf16; the four biases stay general fp32 (the layer
    keeps fp32 masters and rounds them where it uses them).  Scaled so that h, the messages, Z and out are all of order 1."""
    g = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=g)
    E = ei.shape[1]
    x, ea = bfr(rnd(n, Ci)), bfr(torch.rand(E, G, generator=g))
    w1, b1 = bfr(rnd(D3, G) * (2.0 / G ** 0.5)), rnd(D3) * 0.1
    w2, b2 = bfr(rnd(Ci * Co, D3) * (1.5 / (D3 * Ci) ** 0.5)), rnd(Ci * Co) * (0.5 / Ci ** 0.5)
    wr, b = bfr(rnd(Co, Ci) / Ci ** 0.5), rnd(Co) * 0.1
    return dict(x=x, ea=ea, ei=ei, w1=w1, b1=b1, w2=w2, b2=b2, wr=wr, b=b, gout=bfr(rnd(n, Co)))


def _edge_net(w1, b1, w2, b2):
    net = torch.nn.Sequential(torch.nn.Linear(w1.shape[1], w1.shape[0]), torch.nn.ReLU(), torch.nn.Linear(w2.shape[1], w2.shape[0]))
    with torch.no_grad():
        net[0].weight.copy_(w1); net[0].bias.copy_(b1); net[2].weight.copy_(w2); net[2].bias.copy_(b2)
    return net


def load_layer(conv, w1, b1, w2, b2, wr, b, **_):
    """the case's parameters into an NNConv (oracle.ops.NNConv or matdeeplearn_amd.nn.NNConv) built on _edge_net's layout"""
    with torch.no_grad():
        for p, v in ((conv.nn[0].weight, w1), (conv.nn[0].bias, b1), (conv.nn[2].weight, w2), (conv.nn[2].bias, b2),
                     (conv.lin.weight, wr), (conv.bias, b)):
            p.copy_(v)
    return conv


def layer_grads(conv, x):
    return dict(dx=x.grad, dW_nn0=conv.nn[0].weight.grad, db_nn0=conv.nn[0].bias.grad, dW_nn2=conv.nn[2].weight.grad,
                db_nn2=conv.nn[2].bias.grad, dW_root=conv.lin.weight.grad, db=conv.bias.grad)


def layer_reference64(x, ea, ei, w1, b1, w2, b2, wr, b, gout, aggr="mean"):
    """oracle.ops.NNConv(...).double() — it builds the per-edge Ci x Co matrices like the reference does — on the inputs as
    stored, loss = sum(out * gout)"""
    Co, Ci = wr.shape
    conv = load_layer(oops.NNConv(Ci, Co, _edge_net(w1, b1, w2, b2), aggr=aggr), w1, b1, w2, b2, wr, b).double()
    x64 = x.double().requires_grad_(True)
    out = conv(x64, ei, ea.double())
    (out * gout.double()).sum().backward()
    return dict(out=out.detach(), **layer_grads(conv, x64))


def layer_reassociated64(x, ea, ei, w1, b1, w2, b2, wr, b, gout, aggr="mean"):
    """The same layer in fp64 in the re-associated form m_e = Y[src_e] . h_e + Z[src_e] (nn.py:299-303) under autograd: no
    E x Ci x Co tensor.  test_nnconv_budget_host.py shows it equal to layer_reference64 to 1e-12."""
    (Co, Ci), D3, n = wr.shape, w1.shape[0], x.shape[0]
    p = {k: v.double().requires_grad_(True) for k, v in dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, wr=wr, b=b).items()}
    src, tgt = ei[0], ei[1]
    h = torch.relu(ea.double() @ p["w1"].t() + p["b1"])
    Y = p["x"] @ p["w2"].view(Ci, Co * D3)
    m = torch.bmm(Y.index_select(0, src).view(-1, Co, D3), h.unsqueeze(-1)).squeeze(-1)
    m = m + (p["x"] @ p["b2"].view(Ci, Co)).index_select(0, src)
    out = oops.scatter(m, tgt, 0, n, aggr) + p["x"] @ p["wr"].t() + p["b"]
    (out * gout.double()).sum().backward()
    return dict(out=out.detach(), dx=p["x"].grad, dW_nn0=p["w1"].grad, db_nn0=p["b1"].grad, dW_nn2=p["w2"].grad,
                db_nn2=p["b2"].grad, dW_root=p["wr"].grad, db=p["b"].grad)


def layer_model(x, ea, ei, w1, b1, w2, b2, wr, b, gout, aggr="mean", mutation=None, probes=None):
    """nn.NNConv.forward (matdeeplearn_amd/nn.py:335-364) and its backward in plain fp32 torch on the CPU, rounded to bf16 where
    the bf16 layer rounds and nowhere else.  Operands are bf16 values, sums fp32.  Paths below matdeeplearn_amd/:

    forward
      F1  h = bf16(relu(ea bf16(W1)^T + bf16(b1))): one fused dense layer, bias and ReLU on the fp32
          accumulators, one rounding on store                                          nn.py:345, csrc/linear.hip:108,289-295
      F2  Y = bf16(x bf16(W2).view(Ci, Co * D3)): the library product, or mdl_linear_wide (the same
          kernel without bias and activation) for n >= 1024 and Co * D3 >= 640            nn.py:347-348, ops.py:1949-1955
      F3  m = bf16(Y[src] . h)                                                            nn.py:349, csrc/nnconv.hip:301 (k7_model)
      F4  bf16(sum_e m / count) (mean: a division of the fp32 sum)                        nn.py:353, csrc/segment.hip:46,133,180
      F5  Z = bf16(x bf16(b2).view(Ci, Co)): library product                              nn.py:359
      F6  bf16(sum_e Z[src] * (1 / count)) (mean: a multiplication by the fp32 reciprocal) nn.py:359, csrc/gather.hip:149-150
      F7  the bf16 add F4 + F6                                                            nn.py:359
      F8  bf16(x bf16(W_root)^T), F9 the bf16 add F7 + F8                                 nn.py:361, csrc/linear.hip:295
      F10 the bf16 add of bf16(b)                                                         nn.py:363
    backward (g = grad_out, handed unchanged through the three adds)
      B1  db = bf16(column sums of g): autograd's reduction of the broadcast bias add, in bf16
      B2  dW_root = g^T x in fp32 (TN GEMM or the one-pass dense backward); the root's
          input gradient bf16(g bf16(W_root))                                             ops.py:1766-1778
      B3  gz = bf16(g / count) (mean), dZ = bf16(by-source sums of gz[tgt])               ops.py:1174-1176,1206, csrc/gather.hip:150
      B4  db_nn2 = bf16(x^T dZ), input gradient bf16(dZ B2^T): library products           nn.py:359
      B5  dm = bf16(g[tgt] / count) (mean)                                                csrc/segment.hip:67,204
      B6  dh = bf16(Y[src]^T . dm), dY = bf16(sum_e dm (x) h)                             csrc/nnconv.hip:372,396,415 (k7_model)
      B7  dW_nn2 = bf16(x^T dY), input gradient bf16(dY W2r^T): the two products of
          _LinearWide.backward / of autograd's matmul, both library products in bf16      ops.py:1944-1945
      B8  dW_nn0 = (dh .* [h > 0])^T ea, db_nn0 its column sums: fp32, the ReLU mask
          applied to the bf16 dh while the TN GEMM stages it                              ops.py:1768-1769,1671
      B9  dx = bf16(bf16(root's + Z's) + Y's): autograd adds the three bf16 input
          gradients in the order their nodes run (latest forward node first)
    mutation: a key of LAYER_MUTATIONS (applied around `probes` = (probe, hub33)), or None."""
    (Co, Ci), D3, n, E = wr.shape, w1.shape[0], x.shape[0], ei.shape[1]
    f32 = torch.float32
    src, tgt = ei[0], ei[1]
    mut = LAYER_MUTATIONS[mutation][0](ei, n, probes) if mutation else {}
    one = torch.ones(E, dtype=f32)
    mean = aggr == "mean"
    cnt = torch.zeros(n, dtype=f32).index_add_(0, tgt, one).clamp(min=1)
    cnt_f = cnt + mut["cnt_fwd"] if "cnt_fwd" in mut else cnt
    by = lambda idx, v: torch.zeros(n, v.shape[1], dtype=f32).index_add_(0, idx, v)
    col = lambda v: v.view(-1, 1)

    h = bfr(torch.relu(ea @ bfr(w1).t() + bfr(b1)))                                                 # F1
    w2r = bfr(w2).view(Ci, Co * D3)
    Y = bfr(x @ w2r)                                                                                # F2
    m = bfr(k7_contract(Y, h, torch.zeros(E, Co), ei, n, Co, D3, f32)["m"])                         # F3
    s = by(tgt, m * col(mut.get("keep_fwd", one)))
    agg = bfr(s / col(cnt_f)) if mean else bfr(s)                                                   # F4
    B2 = bfr(b2).view(Ci, Co)
    Z = bfr(x @ B2)                                                                                 # F5
    sz = by(tgt, Z.index_select(0, src) * col(mut.get("keep_z", one)))
    zagg = bfr(sz * col(1.0 / cnt_f)) if mean else bfr(sz)                                          # F6
    out = bfr(bfr(bfr(agg + zagg) + bfr(x @ bfr(wr).t())) + bfr(b))                                 # F7 - F10

    g = gout
    db = bfr(g.sum(0))                                                                              # B1
    dW_root, dx_root = g.t() @ x, bfr(g @ bfr(wr))                                                  # B2
    gz = bfr(g / col(cnt)) if mean else g
    dZ = bfr(by(src, gz.index_select(0, tgt)))                                                      # B3
    db_nn2, dx_z = bfr(x.t() @ dZ).reshape(-1), bfr(dZ @ B2.t())                                    # B4
    dm = (bfr(g / col(cnt)) if mean else g).index_select(0, tgt) * col(mut.get("keep_bwd", one))    # B5
    k7 = k7_contract(Y, h, dm, ei, n, Co, D3, f32)
    dh, dY = bfr(k7["dh"]), bfr(k7["dY"])                                                           # B6
    dW_nn2, dx_y = bfr(x.t() @ dY).view(Ci * Co, D3), bfr(dY @ w2r.t())                             # B7
    dpre = dh * (h > 0).to(f32)
    dW_nn0, db_nn0 = dpre.t() @ ea, dpre.sum(0)                                                     # B8
    dx = bfr(bfr(dx_root + dx_z) + dx_y)                                                            # B9
    return dict(out=out, dx=dx, dW_nn0=dW_nn0, db_nn0=db_nn0, dW_nn2=dW_nn2, db_nn2=db_nn2, dW_root=dW_root, db=db)


def _probe_in_edge(ei, probe, which=5):
    """the `which`-th in-edge (stable by-target order) of the probe node whose source is not the probe itself"""
    order = torch.sort(ei[1], stable=True).indices
    own = [int(e) for e in order if int(ei[1, e]) == probe and int(ei[0, e]) != probe]
    return own[min(which, len(own) - 1)]


def _keep(ei, edges):
    k = torch.ones(ei.shape[1], dtype=torch.float32)
    k[edges] = 0.0
    return k


def _mut_divisor(ei, n, probes):
    c = torch.zeros(n, dtype=torch.float32)
    c[probes[0]] = 1.0
    return {"cnt_fwd": c}


FWD_, BWD_ = ("out",), ("dx", "dW_nn0", "db_nn0", "dW_nn2")
# name -> (edit, the tensors the mutated pass writes: the witness may only be one of those)
LAYER_MUTATIONS = {
    "mean_divisor_off_by_one": (_mut_divisor, FWD_),                                    # at the degree-13 probe, forward
    "z_dropped_for_one_source": (lambda ei, n, p: {"keep_z": _keep(ei, (ei[0] == p[1]).nonzero().flatten())}, FWD_),   # the 33-hub
    "edge_dropped_forward": (lambda ei, n, p: {"keep_fwd": _keep(ei, [_probe_in_edge(ei, p[0])])}, FWD_),
    "edge_dropped_backward": (lambda ei, n, p: {"keep_bwd": _keep(ei, [_probe_in_edge(ei, p[0])])}, BWD_),
}


def layer_applies(mutation, aggr):
    return mutation != "mean_divisor_off_by_one" or aggr == "mean"


def layer_ratios(got, model, ref64, names=LAYER_TENSORS):
    return {k: row_ratio(got[k], model[k], ref64[k]) for k in names}


def wide_launch_shape(n, Ci, Co, D3):
    """(mdl_linear_wide takes Y = x W2r, kp, column blocks, width of the last block): ops.matmul_wide's condition (ops.py:1949-1955)
    and the launch arithmetic of csrc/linear.hip (192-column blocks, K padded to a multiple of 64), restated"""
    M = Co * D3
    wide = n >= 1024 and Ci % 2 == 0 and 4 <= Ci <= 160 and M >= 640
    blocks = -(-M // 192)
    return wide, -(-Ci // 64) * 64, blocks, M - 192 * (blocks - 1)


# name -> (n, Ci, Co, D3, aggr, graph keywords)
LAYER_CASES = {
    "layer_small": (100, 20, 36, 50, "mean", {}),                    # library x @ w: the regime of the older parity test
    "layer_wide_24": (1100, 24, 24, 28, "mean", {}),                 # Co * D3 = 672: mdl_linear_wide, kp 64, last block 96 wide
    "layer_wide_100": (1100, 100, 100, 100, "mean", {"max_in": 3}),  # kp 128, 53 column blocks, the last 16 wide; E near 3500
    "layer_add": (100, 20, 36, 50, "add", {}),
}
REASSOCIATED = ("layer_wide_100",)               # fp64 reference in the re-associated form (E x Ci x Co = 3.5e7 doubles otherwise)
LAYER_SEED_SHIFT = {}


@functools.lru_cache(maxsize=None)
def layer_case(name):
    """dict(inputs, probes, aggr, ref, model, ...) of a named layer-level case; shared, read-only"""
    n, Ci, Co, D3, aggr, gkw = LAYER_CASES[name]
    seed = sorted(LAYER_CASES).index(name)
    ei, probe, hub33, hub100, zeros = nn_graph(n, seed=seed, **gkw)
    inp = layer_inputs(ei, n, Ci, Co, D3, seed=300 + seed + 1000 * LAYER_SEED_SHIFT.get(name, 0))
    ref = (layer_reassociated64 if name in REASSOCIATED else layer_reference64)(aggr=aggr, **inp)
    return dict(inputs=inp, probes=(probe, hub33), aggr=aggr, ref=ref, model=layer_model(aggr=aggr, **inp), n=n, Ci=Ci, Co=Co,
                D3=D3, E=ei.shape[1])


def layer_mutated(name, mutation):
    c = layer_case(name)
    return layer_model(aggr=c["aggr"], mutation=mutation, probes=c["probes"], **c["inputs"])
