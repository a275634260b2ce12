"""CPU checks behind the SchNet force path: the reference (oracle.models.SchNet under autograd) against central differences, the
per-edge gradient formulas csrc/cfconv_de.hip implements against autograd of oracle.ops.CFConv, and the public surface
(supported models named in the error, the new entry points declared).  Geometry helpers: tests/test_forces_host.py."""
import math
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import models as omodels
from oracle import ops as oops
from test_forces_host import DS, _toy, edge_dist, edge_shifts

LN2 = math.log(2.0)


def cfconv_edge_grads(rbf, c, h, g, src, tgt, w1, b1, w2, b2):
    """dc [E], dr [E, G] of  out_i = sum_{e: j -> i} h_j * W_e * c_e,  W_e = W2 ssp(W1 r_e + b1) + b2,  for g = dL/dout — the
    formulas of the issue / csrc/cfconv_de.hip written out (the GPU tests' second reference)."""
    pre = rbf @ w1.t() + b1
    a = torch.nn.functional.softplus(pre) - LN2
    w = a @ w2.t() + b2
    q = g.index_select(0, tgt) * h.index_select(0, src)
    dc = (q * w).sum(1)
    da = ((c.unsqueeze(1) * q) @ w2) * torch.sigmoid(pre)
    return dc, da @ w1


def collapse_through_expansion(dr, dn, rbf, offsets, coeff):
    """ddn_e = sum_g dr_e[g] * 2 coeff (dn_e - mu_g) r_e[g]"""
    return (dr * (2.0 * coeff) * (dn.unsqueeze(1) - offsets.unsqueeze(0)) * rbf).sum(1)


def test_oracle_schnet_forces_match_central_differences_fp64():
    """protocol and bound of test_forces_host.test_oracle_forces_match_central_differences_fp64 (h = 1e-5, 1e-5 relative) on a
    toy batch with self loops and a non-orthogonal cell; BatchNorm statistics moved by two optimizer steps"""
    pos, node_ptr, cell, pbc, src, tgt, batch = _toy()
    assert (src == tgt).any() and abs(cell[1][1, 0]) > 0
    sh = torch.from_numpy(edge_shifts(pos, node_ptr, cell, pbc, src, tgt))
    s, t = torch.from_numpy(src), torch.from_numpy(tgt)
    torch.manual_seed(5)
    model = omodels.SchNet(DS(), dim1=16, dim2=16, dim3=16, gc_count=3, post_fc_count=1, cutoff=8).double()
    x = torch.rand(pos.shape[0], 20, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    lo, hi = 0.0, 8.0

    def batch_of(p):
        d = edge_dist(p, sh, s, t)
        return types.SimpleNamespace(x=x, edge_index=torch.stack([s, t]), edge_weight=d,
                                     edge_attr=oops.rbf_expand((d - lo) / (hi - lo), 0.0, 1.0, 16), batch=torch.from_numpy(batch), num_graphs=3)

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    model.train()
    y = torch.randn(3, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    for _ in range(2):
        opt.zero_grad()
        torch.nn.functional.l1_loss(model(batch_of(torch.from_numpy(pos))), y).backward()
        opt.step()
    model.eval()
    assert all(float(bn.running_mean.abs().max()) > 0 for bn in model.bn_list)

    energy = lambda p: model(batch_of(p)).sum()
    p = torch.from_numpy(pos).requires_grad_(True)
    (g,) = torch.autograd.grad(energy(p), p)
    h, fd = 1e-5, np.zeros_like(pos)
    with torch.no_grad():
        for i in range(pos.shape[0]):
            for k in range(3):
                qp, qm = pos.copy(), pos.copy()
                qp[i, k] += h
                qm[i, k] -= h
                fd[i, k] = (float(energy(torch.from_numpy(qp))) - float(energy(torch.from_numpy(qm)))) / (2 * h)
    scale = np.abs(fd).max()
    assert scale > 0
    assert np.abs(g.numpy() - fd).max() <= 1e-5 * scale, (np.abs(g.numpy() - fd).max(), scale)
    for b in range(3):
        assert np.abs(g.numpy()[batch == b].sum(0)).max() <= 1e-12 * max(scale, 1.0)


def test_per_edge_formulas_match_autograd_of_the_oracle_cfconv():
    gen = torch.Generator().manual_seed(11)
    N, E, C, F, G, cutoff = 9, 40, 12, 10, 16, 8.0
    torch.manual_seed(3)
    blk = oops.InteractionBlock(C, G, F, cutoff).double()
    for q in blk.parameters():                            # biases are zero-initialised: move them
        q.data.add_(0.1 * torch.randn(q.shape, dtype=torch.float64, generator=gen))
    conv = blk.conv
    src, tgt = torch.randint(0, N, (E,), generator=gen), torch.randint(0, N, (E,), generator=gen)
    x = torch.randn(N, C, dtype=torch.float64, generator=gen)
    d = (torch.rand(E, dtype=torch.float64, generator=gen) * 7.5).requires_grad_(True)
    dn = (d.detach() / 8.0).requires_grad_(True)
    offsets, coeff = oops.rbf_offsets(0.0, 1.0, G).double(), oops.rbf_coeff(0.0, 1.0, 0.2)
    rbf = oops.rbf_expand(dn, 0.0, 1.0, G)
    rbf.retain_grad()
    gout = torch.randn(N, C, dtype=torch.float64, generator=gen)
    out = conv(x, torch.stack([src, tgt]), d, rbf)
    (out * gout).sum().backward()

    with torch.no_grad():
        g = gout @ conv.lin2.weight                       # dL/d(aggregated messages)
        h = conv.lin1(x)
        c = 0.5 * (torch.cos(d * math.pi / cutoff) + 1.0)
        dc, dr = cfconv_edge_grads(rbf, c, h, g, src, tgt, blk.mlp[0].weight, blk.mlp[0].bias, blk.mlp[2].weight, blk.mlp[2].bias)
        ddn = collapse_through_expansion(dr, dn, rbf, offsets, coeff)
        dd_cut = dc * (-math.pi / (2 * cutoff)) * torch.sin(math.pi * d / cutoff)
    assert torch.allclose(dr, rbf.grad, rtol=1e-10, atol=1e-12 * float(rbf.grad.abs().max()))
    assert torch.allclose(ddn, dn.grad, rtol=1e-10, atol=1e-12 * float(dn.grad.abs().max()))
    assert torch.allclose(dd_cut, d.grad, rtol=1e-10, atol=1e-12 * float(d.grad.abs().max()))
    assert float(d.grad.abs().max()) > 0 and float(dn.grad.abs().max()) > 0


def test_energy_and_forces_names_both_supported_models():
    from matdeeplearn_amd import forces, models, ops
    with pytest.raises(ops.MdlError) as e:
        forces.energy_and_forces(models.GCN(DS(), dim1=16, dim2=16, gc_count=1), [], (0.0, 8.0))
    assert "CGCNN" in str(e.value) and "SchNet" in str(e.value)


def test_new_entry_points_are_declared_in_table_and_header():
    from matdeeplearn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mdl_hip.h")).read()
    for name in ("mdl_cfconv_bwd_edge", "mdl_cfconv_bwd_edge_supported", "mdl_edge_dot"):
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\b%s\(" % name, header), name
    src = open(os.path.join(root, "matdeeplearn_amd", "csrc", "cfconv_de.hip")).read()
    assert "v_mfma_f32_32x32x16_bf16".replace("v_", "__builtin_amdgcn_") in src and "__builtin_amdgcn_mfma_f32_32x32x2f32" in src
