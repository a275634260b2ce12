"""Host checks of the fused Set2Set readout's REFERENCE and of its public surface.  csrc/set2set.hip implements the backward
recurrence written out in set2set_backward below (fp64 here); that transcription is pinned against autograd through
oracle.ops.set2set_loop before any device is involved.  tests/test_gpu_set2set.py leans on loop_reference.  No GPU."""
import os
import re

import pytest
import torch

from oracle import ops as oops


def segments(sizes):
    """sorted node -> graph map of graphs with these node counts (0 = a graph without nodes)"""
    return torch.cat([torch.full((n,), g, dtype=torch.int64) for g, n in enumerate(sizes)])


def loop_reference(x, batch, num_graphs, w_ih, w_hh, b_ih, b_hh, steps):
    """oracle.ops.set2set_loop for a batch that may hold graphs WITHOUT nodes (the loop takes the maximum of the graph's scores,
    which an empty graph does not have): such a graph is given one all-zero row — score 0, weight 1, r = 0, exactly the empty
    sum — whose gradient nobody reads.  Differentiable in x and the parameters."""
    count = torch.bincount(batch, minlength=num_graphs)
    empty = torch.nonzero(count == 0).flatten()
    xa = torch.cat([x, x.new_zeros(empty.numel(), x.shape[1])])
    ba = torch.cat([batch, empty])
    return oops.set2set_loop(xa, ba, w_ih, w_hh, b_ih, b_hh, steps)


def set2set_forward_saved(x, batch, B, w_ih, w_hh, b_ih, b_hh, steps):
    """(out, saved state per step) of Set2Set with the LSTM cell written out, all graphs at once, no autograd"""
    C = x.shape[1]
    qs, h, c = x.new_zeros(B, 2 * C), x.new_zeros(B, C), x.new_zeros(B, C)
    saved = []
    for _ in range(steps):
        G = qs @ w_ih.T + b_ih + h @ w_hh.T + b_hh
        i, f, g, o = torch.sigmoid(G[:, :C]), torch.sigmoid(G[:, C:2 * C]), torch.tanh(G[:, 2 * C:3 * C]), torch.sigmoid(G[:, 3 * C:])
        c_prev, qs_prev, h_prev = c, qs, h
        c = f * c + i * g
        q = h = o * torch.tanh(c)
        e = (x * q[batch]).sum(1)
        emax = torch.full((B,), float("-inf"), dtype=x.dtype).scatter_reduce(0, batch, e, "amax", include_self=True)
        p = torch.exp(e - emax[batch])
        a = p / (torch.zeros(B, dtype=x.dtype).index_add_(0, batch, p)[batch] + 1e-16)
        r = torch.zeros(B, C, dtype=x.dtype).index_add_(0, batch, a[:, None] * x)
        qs = torch.cat([q, r], 1)
        saved.append(dict(i=i, f=f, g=g, o=o, c=c, c_prev=c_prev, q=q, r=r, a=a, qs_prev=qs_prev, h_prev=h_prev))
    return qs, saved


def set2set_backward(x, batch, B, w_ih, w_hh, saved, gout):
    """The recurrence the device kernel walks, t = T..1:
        [dq | dr] = dq*_t (+ dh carried);  da_n = <dr, x_n>;  s = sum a_n da_n;  de_n = a_n (da_n - s)
        dq += sum_n de_n x_n;  dx_n += a_n dr + de_n q_t;  LSTM cell backward -> dG_t, dc_{t-1}
        dq*_{t-1} = W_ih^T dG_t;  dh_{t-1} = W_hh^T dG_t
    and the parameter gradients as sums over the steps.  Returns dG [T, B, 4C], dx, dW_ih, dW_hh, db_ih, db_hh."""
    C = x.shape[1]
    dqs, dh, dc = gout.clone(), torch.zeros(B, C, dtype=x.dtype), torch.zeros(B, C, dtype=x.dtype)
    dx = torch.zeros_like(x)
    dG_all = []
    dw_ih, dw_hh, db = torch.zeros_like(w_ih), torch.zeros_like(w_hh), torch.zeros(4 * C, dtype=x.dtype)
    for sv in reversed(saved):
        dq, dr = dqs[:, :C] + dh, dqs[:, C:]
        da = (x * dr[batch]).sum(1)
        s = torch.zeros(B, dtype=x.dtype).index_add_(0, batch, sv["a"] * da)
        de = sv["a"] * (da - s[batch])
        dq = dq + torch.zeros(B, C, dtype=x.dtype).index_add_(0, batch, de[:, None] * x)
        dx = dx + sv["a"][:, None] * dr[batch] + de[:, None] * sv["q"][batch]
        th = torch.tanh(sv["c"])
        dcc = dc + dq * sv["o"] * (1 - th * th)
        dG = torch.cat([dcc * sv["g"] * sv["i"] * (1 - sv["i"]), dcc * sv["c_prev"] * sv["f"] * (1 - sv["f"]),
                        dcc * sv["i"] * (1 - sv["g"] ** 2), dq * th * sv["o"] * (1 - sv["o"])], 1)
        dc = dcc * sv["f"]
        dG_all.append(dG)
        dw_ih += dG.T @ sv["qs_prev"]
        dw_hh += dG.T @ sv["h_prev"]
        db += dG.sum(0)
        dqs, dh = dG @ w_ih, dG @ w_hh
    return torch.stack(dG_all[::-1]), dx, dw_ih, dw_hh, db, db.clone()


def lstm_params(C, seed, dtype=torch.float64):
    torch.manual_seed(seed)
    L = oops.Set2Set(C, processing_steps=1).lstm
    return [p.detach().to(dtype).clone() for p in (L.weight_ih_l0, L.weight_hh_l0, L.bias_ih_l0, L.bias_hh_l0)]


def _close(a, b, what):
    scale = float(b.abs().max())
    assert scale > 0, what
    assert float((a - b).abs().max()) <= 1e-10 * scale, (what, float((a - b).abs().max()), scale)


@pytest.mark.parametrize("C", [1, 5])
def test_backward_recurrence_matches_autograd_through_the_loop_fp64(C):
    sizes, T = [1, 2, 7, 0, 13], 3
    B, batch = len(sizes), segments(sizes)
    gen = torch.Generator().manual_seed(10 + C)
    x = torch.randn(sum(sizes), C, dtype=torch.float64, generator=gen).requires_grad_(True)
    gout = torch.randn(B, 2 * C, dtype=torch.float64, generator=gen)
    params = [p.requires_grad_(True) for p in lstm_params(C, C)]
    out = loop_reference(x, batch, B, *params, T)
    auto = torch.autograd.grad((out * gout).sum(), [x] + params)
    with torch.no_grad():
        mine, saved = set2set_forward_saved(x, batch, B, *params, T)
        dG, dx, dw_ih, dw_hh, db_ih, db_hh = set2set_backward(x, batch, B, params[0], params[1], saved, gout)
    _close(mine, out.detach(), "out")
    assert float(saved[-1]["r"][3].abs().max()) == 0.0                   # the graph without nodes
    assert torch.equal(saved[-1]["r"][0], x.detach()[0])                 # one node: r = x
    for got, want, what in zip((dx, dw_ih, dw_hh, db_ih, db_hh), auto, ("dx", "dw_ih", "dw_hh", "db_ih", "db_hh")):
        _close(got, want, what)
    # dG: autograd sees it through a bias of the graph's own — the gradient of graph s's private b_ih is sum_t dG_t[s]
    per_graph = []
    for s in range(B):
        bs = params[2].detach().clone().requires_grad_(True)
        xs = x.detach()[batch == s]
        o = loop_reference(xs, torch.zeros(xs.shape[0], dtype=torch.int64), 1, params[0].detach(), params[1].detach(), bs,
                           params[3].detach(), T)
        per_graph.append(torch.autograd.grad((o[0] * gout[s]).sum(), bs)[0])
    _close(dG.sum(0), torch.stack(per_graph), "sum_t dG_t per graph")


@pytest.mark.parametrize("C", [1, 5])
def test_single_step_gate_gradient_is_the_bias_gradient_per_graph_fp64(C):
    """T = 1: dG_1[s] itself is what autograd gives a per-graph bias; W_ih and W_hh get no gradient (q*_0 = h_0 = 0)"""
    sizes = [1, 2, 7, 0, 13]
    B, batch = len(sizes), segments(sizes)
    gen = torch.Generator().manual_seed(20 + C)
    x = torch.randn(sum(sizes), C, dtype=torch.float64, generator=gen)
    gout = torch.randn(B, 2 * C, dtype=torch.float64, generator=gen)
    params = lstm_params(C, 3 + C)
    _, saved = set2set_forward_saved(x, batch, B, *params, 1)
    dG, _, dw_ih, dw_hh, _, _ = set2set_backward(x, batch, B, params[0], params[1], saved, gout)
    assert float(dw_ih.abs().max()) == 0.0 and float(dw_hh.abs().max()) == 0.0
    for s in range(B):
        bs = params[2].clone().requires_grad_(True)
        xs = x[batch == s]
        o = loop_reference(xs, torch.zeros(xs.shape[0], dtype=torch.int64), 1, params[0], params[1], bs, params[3], 1)
        _close(dG[0, s], torch.autograd.grad((o[0] * gout[s]).sum(), bs)[0], "dG_1[%d]" % s)


# ---------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------
def test_set2set_entry_points_are_declared_in_table_header_and_library():
    from matdeeplearn_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mdl_hip.h")).read()
    for name in ("mdl_set2set_supported", "mdl_set2set_fwd", "mdl_set2set_bwd"):
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\b%s\(" % name, header), name
        if os.path.exists(_build.LIB):
            assert hasattr(_lib.lib(), name), name


def test_supported_shapes_cover_every_width_and_step_count_of_the_contract():
    from matdeeplearn_amd import _build, _lib
    if not os.path.exists(_build.LIB):
        return                                    # (checked where the library is built, like the entry points above)
    fn = _lib.lib().mdl_set2set_supported
    for dt in (_lib.MDL_F32, _lib.MDL_BF16):
        assert all(fn(C, T, dt) == 1 for C in range(1, 129) for T in range(1, 9))
        assert fn(0, 3, dt) == 0 and fn(129, 3, dt) == 0 and fn(64, 0, dt) == 0 and fn(64, 9, dt) == 0
    assert fn(64, 3, 7) == 0


def test_ops_surface_has_the_option_and_the_operator():
    from matdeeplearn_amd import ops
    assert "set2set_fused" in ops.OPTIONS
    assert ops.options()["set2set_fused"] is True
    assert callable(ops.set2set) and callable(ops.set2set_fused_ok)
    prev = ops.configure(set2set_fused=False)
    try:
        assert prev == {"set2set_fused": True} and ops.options()["set2set_fused"] is False
    finally:
        ops.configure(**prev)
