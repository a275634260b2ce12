"""bf16 NNConv on the device against the fp64 reference, per row, within ALLOWED times the error of the rounding model
(tests/nnconv_budget.py).
Op level: K7 alone (csrc/nnconv.hip) through the C ABI on every route of its dispatch — the flat staging of Y_j with five and
with seven chunks per thread and at the boundaries between them, the fallbacks for shape and for alignment, the scalar kernels in
bf16 with their second accumulator pass, eid_s = NULL — with the outputs carved out of a NaN-filled arena: what the kernels must
not write stays NaN, the dY rows of nodes without out-edges are exactly zero.
Layer level: nn.NNConv forward and backward, with Y = x W2r from the library and from the streaming kernel (mdl_linear_wide).
test_nnconv_budget_host.py shows that these checks can fail: every mutation of the model stands at least 2 x ALLOWED over it."""
import pytest
import torch

import nnconv_budget as B

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _report(name, route, r):
    print("[budget] %-18s %-28s %s" % (name, route, "  ".join("%s %.4f" % kv for kv in r.items())))
    over = {k: v for k, v in r.items() if not v <= B.ALLOWED[k]}
    assert not over, "%s %s: over the budget %s: %s" % (name, route, {k: B.ALLOWED[k] for k in over}, over)


def _route_label(route):
    kind, ff, bf, maxc = route
    return kind if kind == "scalar" else "mfma fwd %s bwd %s <%d>" % ("flat" if ff else "dense", "flat" if bf else "dense", maxc)


# ---------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------
class _Arena:
    """bf16 outputs carved out of ONE NaN-filled allocation, GUARD bytes behind each; every output starts `off` bytes past a
    16-byte boundary"""

    def __init__(self, specs, d):
        g = B.GUARD // 2
        self.spans, pos = {}, 0
        for name, rows, cols, off in specs:
            assert off % 2 == 0
            pos = (pos + 7) // 8 * 8 + off // 2
            self.spans[name] = (pos, rows, cols)
            pos += rows * cols + g
        self.buf = torch.full((pos + 8,), float("nan"), dtype=torch.bfloat16, device=d)
        assert self.buf.data_ptr() % 16 == 0

    def view(self, name):
        pos, rows, cols = self.spans[name]
        return self.buf[pos:pos + rows * cols].view(rows, cols)

    def outside(self):
        """every element of the allocation that belongs to no output: guards and alignment gaps"""
        mask = torch.ones(self.buf.numel(), dtype=torch.bool)
        for pos, rows, cols in self.spans.values():
            mask[pos:pos + rows * cols] = False
        return self.buf.cpu()[mask]


@pytest.mark.parametrize("name", list(B.OP_CASES))
def test_k7_routes_through_the_c_abi(name):
    from matdeeplearn_amd import _lib
    d, bf16 = dev(), torch.bfloat16
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    c = B.op_case(name)
    i, n, Co, D3, E = c["inputs"], c["n"], c["Co"], c["D3"], c["E"]
    ybuf = torch.empty(n * Co * D3 + 8, dtype=bf16, device=d)
    assert ybuf.data_ptr() % 16 == 0
    Y = ybuf[c["y_off"] // 2:c["y_off"] // 2 + n * Co * D3].view(n, Co * D3)
    Y.copy_(i["Y"])
    h, dm = i["h"].to(d).to(bf16).contiguous(), i["dm"].to(d).to(bf16).contiguous()
    rowptr_s = c["rowptr_s"].to(d)
    eid_s = None if c["eid_s"] is None else c["eid_s"].to(d)
    arena = _Arena([("m", E + B.PAD, Co, 0), ("dh", E + B.PAD, D3, 0), ("dY", n, Co * D3, c["dy_off"])], d)
    m, dh, dY = arena.view("m"), arena.view("dh"), arena.view("dY")
    # the route this call takes, from the pointers it passes
    for t in (h, dm, m, dh):
        assert t.data_ptr() % 4 == 0
    route = B.k7_route(Co, D3, Y.data_ptr() % 16, dY.data_ptr() % 16)
    assert route == c["route"], (name, route)
    assert (eid_s is None) == (name == "by_source_null")

    _lib.check(L.mdl_nnconv_msg_fwd(P(Y), P(h), P(rowptr_s), P(eid_s), P(m), n, Co, D3, _lib.MDL_BF16, st()), "mdl_nnconv_msg_fwd")
    _lib.check(L.mdl_nnconv_msg_bwd(P(Y), P(h), P(dm), P(rowptr_s), P(eid_s), P(dh), P(dY), n, Co, D3, _lib.MDL_BF16, st()),
               "mdl_nnconv_msg_bwd")
    torch.cuda.synchronize()
    got = dict(m=m.cpu().float(), dh=dh.cpu().float(), dY=dY.cpu().float())
    # what the kernels must not write: the padded edge rows, the guards behind every output, the gaps in front
    assert bool(torch.isnan(got["m"][E:]).all()) and bool(torch.isnan(got["dh"][E:]).all()), "a padded edge row was written"
    assert bool(torch.isnan(arena.outside().float()).all()), "a store landed outside m / dh / dY"
    got["m"], got["dh"] = got["m"][:E], got["dh"][:E]
    for k in B.OP_TENSORS:
        assert bool(torch.isfinite(got[k]).all()), k
    outdeg = torch.bincount(i["ei"][0], minlength=n)
    assert [int(outdeg[z]) for z in c["zeros"]] == [0, 0, 0]
    for z in c["zeros"]:
        assert float(got["dY"][z].abs().max()) == 0.0, "dY of node %d (no out-edges) is not zero" % z
    _report(name, _route_label(route), B.op_ratios(got, c["model"], c["ref"], Co, D3))


# ---------------------------------------------------------------------------------------------
# layer level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.LAYER_CASES))
def test_layer_forward_and_backward(name, monkeypatch):
    """nn.NNConv in bf16 on fp32 master parameters, as tests/test_gpu_kernels.test_nnconv_contraction_matches_oracle runs it.
    The wide cases must take Y = x W2r through mdl_linear_wide (once per forward), the small ones through the library."""
    from matdeeplearn_amd import nn as pnn, ops
    d, bf16 = dev(), torch.bfloat16
    c = B.layer_case(name)
    i, n, Ci, Co, D3 = c["inputs"], c["n"], c["Ci"], c["Co"], c["D3"]
    wide, kp, blocks, last = B.wide_launch_shape(n, Ci, Co, D3)
    assert (wide, kp, blocks, last) == {"layer_small": (False, 64, 10, 72), "layer_add": (False, 64, 10, 72),
                                        "layer_wide_24": (True, 64, 4, 96), "layer_wide_100": (True, 128, 53, 16)}[name]
    assert B.k7_route(Co, D3)[0] == "mfma"
    entered = []
    forward = ops._LinearWide.forward

    def counted(ctx, x, w):
        entered.append(tuple(w.shape))
        return forward(ctx, x, w)
    monkeypatch.setattr(ops._LinearWide, "forward", staticmethod(counted))
    monkeypatch.setattr(ops, "KERNEL_EVENTS", {"nnconv_fwd": []})

    conv = B.load_layer(pnn.NNConv(Ci, Co, B._edge_net(i["w1"], i["b1"], i["w2"], i["b2"]), aggr=c["aggr"]), **i).to(d)
    x = i["x"].to(d).to(bf16).requires_grad_(True)
    out = conv(x, i["ei"].to(d), i["ea"].to(d).to(bf16))
    (out.float() * i["gout"].to(d)).sum().backward()
    torch.cuda.synchronize()
    assert out.dtype == bf16 and x.grad.dtype == bf16
    assert entered == ([(Ci, Co * D3)] if wide else []), entered
    assert len(ops.KERNEL_EVENTS["nnconv_fwd"]) == 1
    got = {k: v.detach().cpu().float() for k, v in dict(out=out, **B.layer_grads(conv, x)).items()}
    for k in B.LAYER_TENSORS:
        assert got[k].shape == c["ref"][k].shape and bool(torch.isfinite(got[k]).all()), k
    _report(name, "linear_wide kp %d, %d blocks" % (kp, blocks) if wide else "library x @ w", B.layer_ratios(got, c["model"], c["ref"]))
