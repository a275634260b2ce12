"""bf16 CFConv on the device against the fp64 reference, per row, within ALLOWED times the error of the rounding model
(tests/cfconv_budget.py): K4 (csrc/cfconv.hip), dh (K4 on the by-source CSR), K4b (csrc/cfconv_bwd.hip) in its three flush forms
and K4d (csrc/cfconv_de.hip) with its three launch forms, through the routes a SchNet block takes — nn.CFConv.aggregate with
recomputed or stored activations, ops.cfconv for the per-edge gradients — at every tail shift of the last 32-unit block, with
sources of out-degree 33 and 100, and on a graph long enough for the second tile of a K4d wave and the steady state of K4b's
pipeline.  Every run records the launches and asserts that the kernels meant are the ones that ran.
test_cfconv_budget_host.py shows that these checks can fail: every mutation of the model stands at least 2 x ALLOWED over it."""
import collections

import pytest
import torch

import cfconv_budget as B

pytestmark = pytest.mark.gpu

K4B = ("dW1", "db1", "dW2", "db2")
NODE = ("out", "dh") + K4B
EVENT_KEYS = ("cfconv_fwd", "cfconv_bwd_h", "cfconv_bwd_w", "cfconv_bwd_edge")


def dev():
    return torch.device("cuda:0")


class _Launches:
    """records ops.KERNEL_EVENTS / ops.K4D_LAUNCHES over a block and restores what it touched"""

    def __enter__(self):
        from matdeeplearn_amd import ops
        self.ops, self.prev = ops, ops.KERNEL_EVENTS
        ops.KERNEL_EVENTS = {k: [] for k in EVENT_KEYS}
        self.k4d0 = collections.Counter(ops.K4D_LAUNCHES)
        return self

    def __exit__(self, *exc):
        ops = self.ops
        self.count = tuple(len(ops.KERNEL_EVENTS[k]) for k in EVENT_KEYS[:3])          # (K4, dh, K4b)
        k4d = collections.Counter(ops.K4D_LAUNCHES)
        k4d.subtract(self.k4d0)
        self.k4d = {k: v for k, v in k4d.items() if v}
        assert len(ops.KERNEL_EVENTS["cfconv_bwd_edge"]) == sum(self.k4d.values())
        ops.KERNEL_EVENTS = self.prev
        return False


def _filter_net(c, d):
    i = c["inputs"]
    from matdeeplearn_amd import nn as mnn
    la, lb = torch.nn.Linear(B.G, c["F"]), torch.nn.Linear(c["F"], c["F"])
    with torch.no_grad():
        la.weight.copy_(i["w1"]); la.bias.copy_(i["b1"]); lb.weight.copy_(i["w2"]); lb.bias.copy_(i["b2"])
    return torch.nn.Sequential(la, mnn.ShiftedSoftplus(), lb).to(d)


def _param_grads(net):
    return dict(zip(K4B, (net[0].weight.grad, net[0].bias.grad, net[2].weight.grad, net[2].bias.grad)))


def _cpu(r):
    torch.cuda.synchronize()
    return {k: v.detach().cpu() for k, v in r.items() if v is not None}


def _aggregate(c, cache=None, rbf_grad=False, cut_grad=False, dist=False):
    """nn.CFConv.aggregate forward + backward once on the case's inputs in bf16 -> (dict like reference64's, the launches).
    lin1 is the identity (exact in bf16: one non-zero product per sum), so h = x and dh = x.grad."""
    from matdeeplearn_amd import nn as mnn, ops
    d, bf16, i = dev(), torch.bfloat16, c["inputs"]
    assert c["sorted"]
    net = _filter_net(c, d)
    conv = mnn.CFConv(c["F"], c["F"], c["F"], net, 8.0).to(d)
    with torch.no_grad():
        conv.lin1.weight.copy_(torch.eye(c["F"]))
    conv.lin1.weight.requires_grad_(False)
    x = i["h"].to(d).to(bf16).requires_grad_(True)
    rbf = i["rbf"].to(d).to(bf16).requires_grad_(rbf_grad)
    cut = i["cut"].to(d).requires_grad_(cut_grad)
    dn = i["dn"].to(d).requires_grad_(dist)
    csr = ops.build_csr(i["ei"].to(d), c["n"], assume_sorted=True)
    dist_arg = (dn, ops.rbf_offsets(B.RBF["start"], B.RBF["stop"], B.G, d), ops.rbf_coeff(**B.RBF)) if dist else None
    with _Launches() as ln:
        out = conv.aggregate(x, None, None, rbf, csr=csr, cut=cut, by_source=cache, dist=dist_arg)
        (out.float() * i["gout"].to(d)).sum().backward()
    assert out.dtype == bf16 and x.grad.dtype == bf16
    r = dict(out=out, dh=x.grad, drbf=rbf.grad, dcut=cut.grad, dd=dn.grad, **_param_grads(net))
    return _cpu(r), ln


def _ops_cfconv(c, pad=0, train=True, fn=None):
    """ops.cfconv (or fn) forward + backward with gradients asked of rbf and cut; pad: rows past rowptr[N], NaN in rbf and cut"""
    from matdeeplearn_amd import ops
    d, bf16, i = dev(), torch.bfloat16, c["inputs"]
    net = _filter_net(c, d)
    csr = ops.build_csr(i["ei"].to(d), c["n"], assume_sorted=c["sorted"])
    assert (csr.eperm is None) == c["sorted"]
    rbf, cut = i["rbf"].to(d).to(bf16), i["cut"].to(d)
    if pad:
        fill = torch.zeros(pad, dtype=torch.int32, device=d)
        csr = ops.EdgeCSR(csr.rowptr, torch.cat([csr.src, fill]), torch.cat([csr.tgt, fill]), None, c["n"], c["E"] + pad)
        csr.partial = True
        rbf = torch.cat([rbf, torch.full((pad, B.G), float("nan"), dtype=bf16, device=d)])
        cut = torch.cat([cut, torch.full((pad,), float("nan"), device=d)])
    if not train:
        for q in net.parameters():
            q.requires_grad_(False)
    edge = fn is None
    rbf.requires_grad_(edge)
    cut.requires_grad_(edge)
    h = i["h"].to(d).to(bf16).requires_grad_(train)
    with _Launches() as ln:
        out = ops.cfconv(rbf, cut, h, csr, net[0], net[2]) if edge else fn(rbf, cut, h, csr, net[0], net[2])
        (out.float() * i["gout"].to(d)).sum().backward()
    r = dict(out=out, dh=h.grad, drbf=rbf.grad, dcut=cut.grad)
    if train:
        r.update(_param_grads(net))
    return _cpu(r), ln, (net, csr)


def _check(name, route, label, got, names):
    """prints the ratios of the tensors `names` against the route's model, asserts each <= ALLOWED"""
    c = B.case(name)
    assert set(names) <= set(got), (names, sorted(got))
    r = B.ratios(got, B.model(name, "stored" if route == "stored" else "edge"), c["ref"], c["order"], names)
    assert len(r) == len(names)
    print("[budget] %-20s %-10s %-14s %s" % (name, route, label, "  ".join("%s %.4f" % kv for kv in r.items())))
    over = {k: v for k, v in r.items() if not v <= B.ALLOWED[k]}
    assert not over, "%s %s %s: over the budget %s: %s" % (name, route, label, {k: B.ALLOWED[k] for k in over}, over)
    return r


# ---------------------------------------------------------------------------------------------
# recompute: K4 + dh + K4b
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cached", [False, True])
@pytest.mark.parametrize("F", B.WIDTHS)
def test_recomputing_route_at_every_width(F, cached, monkeypatch):
    """all three instantiations (3, 4, 5 blocks of 32 units), every shift of the h[src] tail in the last block, the last block
    empty (64, 96, 128) or two units wide (66, 130); hub sources of out-degree 33 and 100 in the dh pass"""
    from matdeeplearn_amd import ops
    monkeypatch.setattr(ops, "_CFCONV_RECOMPUTE_MIN_F", 0)
    got, ln = _aggregate(B.case("width%d" % F), cache=ops.BySourceAttrs() if cached else None)
    assert ln.count == (1, 1, 1) and not ln.k4d, (ln.count, ln.k4d)
    _check("width%d" % F, "recompute", "cache" if cached else "no_cache", got, NODE)


@pytest.mark.parametrize("name", ["two_groups_plus_one", "small_cutoffs", "long"])
def test_recomputing_route_group_tail_zero_cutoffs_long_graph(name, monkeypatch):
    """n 65: two 32-node groups plus one node; cutoff factors down to exactly 0; E > 49 152: every K4b workgroup runs the
    steady state of its pipeline (the launch arithmetic of the case is pinned in test_cfconv_budget_host.py)"""
    from matdeeplearn_amd import ops
    monkeypatch.setattr(ops, "_CFCONV_RECOMPUTE_MIN_F", 0)
    if name == "long":
        assert 49152 < B.case(name)["E"] < 70000 and B.long_launch_shape(B.case(name)["E"])[0] >= 3
    got, ln = _aggregate(B.case(name))
    assert ln.count == (1, 1, 1) and not ln.k4d, (ln.count, ln.k4d)
    _check(name, "recompute", "", got, NODE)


def test_single_node():
    """n 1, five self-edges: below the row count the fused training route asks for, so through ops.cfconv_recompute"""
    from matdeeplearn_amd import ops
    c = B.case("single_node")
    assert c["n"] == 1 and c["E"] == 5
    got, ln, _ = _ops_cfconv(c, fn=lambda *a: ops.cfconv_recompute(*a))
    assert ln.count == (1, 1, 1) and not ln.k4d, (ln.count, ln.k4d)
    _check("single_node", "recompute", "", got, NODE)


# ---------------------------------------------------------------------------------------------
# stored activations: K4 writing a1 / w, the backward by the dense and gather nodes
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,default", [(64, True), (66, True), (94, True), (100, False), (150, False)])
def test_stored_activation_route(F, default):
    from matdeeplearn_amd import ops
    name = "width%d" % F
    c = B.case(name)
    assert (F < ops._CFCONV_RECOMPUTE_MIN_F) == default
    prev = ops.configure(cfconv_recompute=default)
    try:
        got, ln = _aggregate(c)
    finally:
        ops.configure(**prev)
    assert ln.count == (1, 0, 0) and not ln.k4d, (ln.count, ln.k4d)
    _check(name, "stored", "default" if default else "recompute_off", got, NODE)
    # the activations K4 stores, against the model's a1 / W (rows = edges); the same launch gives the same out
    d, i = dev(), c["inputs"]
    net = _filter_net(c, d)
    csr = ops.build_csr(i["ei"].to(d), c["n"], assume_sorted=True)
    out, a1, w = ops.cfconv_fused(i["rbf"].to(d).bfloat16(), i["cut"].to(d), i["h"].to(d).bfloat16(), csr, net[0], net[2], want_acts=True)
    assert torch.equal(out.cpu(), got["out"])
    m = B.model(name, "stored")
    for k, v in (("a1", a1), ("w", w)):
        r = B.row_ratio(v.cpu(), m[k], c["ref"][k])
        print("[budget] %-20s %-10s %-14s %s %.4f" % (name, "stored", "activation", k, r))
        assert r <= B.ALLOWED["out"], (k, r)                   # (rounded once on store from fp32 sums, like out)


# ---------------------------------------------------------------------------------------------
# edge: K4d behind K4 + dh + K4b
# ---------------------------------------------------------------------------------------------
EDGE_FORMS = {                                   # form -> (aggregate keywords, K4d launches, the tensors K4d writes)
    "general": (dict(rbf_grad=True, cut_grad=True), {"general": 1}, ("drbf", "dcut")),
    "distance": (dict(dist=True, cut_grad=True), {"distance": 1}, ("dd", "dcut")),
    "dcut_only": (dict(cut_grad=True), {"dcut": 1}, ("dcut",)),
}


@pytest.mark.parametrize("name,form", [(w, f) for w in ("width64", "width100", "width150") for f in EDGE_FORMS]
                         + [(n, f) for n in ("far_sources", "long") for f in ("general", "distance")])
def test_edge_route(name, form):
    """ops.cfconv through nn.CFConv.aggregate with gradients asked of rbf and cut (general epilogue + dcut), of the distance
    and cut (distance epilogue + dcut), of cut alone (the dcut-only launch: the first half of the chain, at the three widths).
    `long`: E > 65 536, every K4d wave runs a second tile behind the LDS fence at the top of its loop."""
    kw, k4d, names = EDGE_FORMS[form]
    if name == "long":
        assert 49152 < B.case(name)["E"] < 70000 and B.long_launch_shape(B.case(name)["E"])[1] >= 2
    got, ln = _aggregate(B.case(name), **kw)
    assert ln.count == (1, 1, 1) and ln.k4d == k4d, (ln.count, ln.k4d)
    _check(name, "edge", form, got, NODE + names)


def test_edge_route_unsorted_edge_list():
    """a shuffled edge list through ops.cfconv: the kernels read CSR-ordered copies, the gradients come back in the caller's
    order; the fused training route refuses an edge permutation"""
    from matdeeplearn_amd import ops
    c = B.case("unsorted")
    got, ln, (net, csr) = _ops_cfconv(c)
    assert ln.count == (1, 1, 1) and ln.k4d == {"general": 1}, (ln.count, ln.k4d)
    i = c["inputs"]
    assert not ops.cfconv_fused_ok(i["rbf"].to(dev()).bfloat16(), i["h"].to(dev()).bfloat16(), csr, net[0], net[2])
    _check("unsorted", "edge", "general", got, NODE + ("drbf", "dcut"))


def test_edge_route_padded_batch():
    """77 rows past rowptr[N] with NaN in rbf and cut: every output finite, the padded rows of drbf / dcut zero"""
    c = B.case("padded")
    got, ln, _ = _ops_cfconv(c, pad=B.PAD, train=False)
    assert ln.count == (1, 0, 0) and ln.k4d == {"general": 1}, (ln.count, ln.k4d)
    E = c["E"]
    assert got["drbf"].shape[0] == E + B.PAD and got["dcut"].shape[0] == E + B.PAD
    for k in ("out", "drbf", "dcut"):
        assert bool(torch.isfinite(got[k].float()).all()), k
    assert float(got["drbf"][E:].float().abs().max()) == 0.0 and float(got["dcut"][E:].abs().max()) == 0.0
    got["drbf"], got["dcut"] = got["drbf"][:E], got["dcut"][:E]
    _check("padded", "edge", "general", got, ("out", "drbf", "dcut"))


# ---------------------------------------------------------------------------------------------
# the flush forms of K4b
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [64, 100, 150])
def test_k4b_flush_forms(F, monkeypatch):
    """default: partial blocks through the scratch buffer + the reduce launch (atomics: measured twice); deterministic: ONE
    workgroup runs every tile, the whole pipeline at small E, bit-equal run to run; scratch = NULL through the C ABI: atomics
    from every workgroup"""
    from matdeeplearn_amd import _lib, ops
    monkeypatch.setattr(ops, "_CFCONV_RECOMPUTE_MIN_F", 0)
    name = "width%d" % F
    c = B.case(name)
    for run in range(2):
        got, ln = _aggregate(c)
        assert ln.count == (1, 1, 1)
        _check(name, "recompute", "scratch_%d" % run, got, K4B)
    with ops.deterministic(True):
        a, ln = _aggregate(c)
        b, _ = _aggregate(c)
    assert ln.count == (1, 1, 1) and not ops._DET
    for k in NODE:
        assert torch.equal(a[k], b[k]), k
    _check(name, "recompute", "deterministic", a, NODE)
    # the atomic form
    d, i = dev(), c["inputs"]
    L, P = _lib.lib(), _lib.ptr
    csr = ops.build_csr(i["ei"].to(d), c["n"], assume_sorted=True)
    t = [i[k].to(d).contiguous() for k in ("w1", "b1", "w2", "b2")]
    wpack = ops._cfconv_pack(*t, F, B.G, d)
    rbf, h, g = (i[k].to(d).bfloat16().contiguous() for k in ("rbf", "h", "gout"))
    cut = i["cut"].to(d).contiguous()
    outs = [torch.zeros(s, dtype=torch.float32, device=d) for s in ((F, B.G), (F,), (F, F), (F,))]
    _lib.check(L.mdl_cfconv_bwd_w(P(rbf), P(cut), P(h), P(g), P(csr.rowptr), P(csr.src), P(csr.tgt), P(wpack), P(outs[0]), P(outs[1]),
                                  P(outs[2]), P(outs[3]), None, c["n"], c["E"], F, B.G, _lib.MDL_BF16, _lib.stream()), "mdl_cfconv_bwd_w")
    _check(name, "recompute", "atomic", _cpu(dict(zip(K4B, outs))), K4B)
