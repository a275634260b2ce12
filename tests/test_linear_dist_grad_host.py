"""CPU checks behind the MEGNet / MPNN force path: the formula csrc/linear_de.hip implements against autograd of the dense layer on
the Gaussian expansion, the references (oracle.models.MEGNet / MPNN under autograd) against central differences, and the public
surface (the new entry points declared and exported, GCN still refused).  Geometry helpers: tests/test_forces_host.py."""
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import models as omodels
from oracle import ops as oops
from test_forces_host import DS, _toy, edge_dist, edge_shifts


def linear_dist_grad(g, w, d, offsets, coeff, act_y=None, scale=1.0):
    """dd[e] = scale * sum_k (sum_c gp[e, c] W[c, k]) * 2 coeff (d_e - mu_k) exp(coeff (d_e - mu_k)^2), gp = g or g * (act_y > 0):
    the formula of the issue / csrc/linear_de.hip written out (the GPU tests' reference)."""
    gp = g if act_y is None else g * (act_y > 0).to(g.dtype)
    diff = d.unsqueeze(1) - offsets.unsqueeze(0)
    return scale * ((gp @ w) * (2.0 * coeff) * diff * torch.exp(coeff * diff * diff)).sum(1)


@pytest.mark.parametrize("E,M,G", [(37, 12, 16), (5, 1, 1), (64, 100, 50)])
def test_formula_matches_autograd_of_the_dense_layer_on_the_expansion_fp64(E, M, G):
    gen = torch.Generator().manual_seed(E + M)
    w = torch.randn(M, G, dtype=torch.float64, generator=gen)
    b = torch.randn(M, dtype=torch.float64, generator=gen)
    d = torch.rand(E, dtype=torch.float64, generator=gen).requires_grad_(True)
    offsets, coeff = oops.rbf_offsets(0.0, 1.0, G).double(), oops.rbf_coeff(0.0, 1.0, 0.2)
    pre = oops.rbf_expand(d, 0.0, 1.0, G) @ w.t() + b
    y = torch.relu(pre)
    g = torch.randn(E, M, dtype=torch.float64, generator=gen)
    (ref,) = torch.autograd.grad((y * g).sum(), d, retain_graph=True)
    with torch.no_grad():
        masked = linear_dist_grad(g, w, d, offsets, coeff, act_y=y)
        handed = linear_dist_grad(g * (pre > 0), w, d, offsets, coeff)          # the derivative handed down: no mask
    assert float(ref.abs().max()) > 0 or M == 1           # (one unit may be dead on every row; the no-activation case below is not)
    assert torch.allclose(masked, ref, rtol=1e-10, atol=1e-12 * float(ref.abs().max()))
    assert torch.allclose(handed, ref, rtol=1e-10, atol=1e-12 * float(ref.abs().max()))
    (ref_lin,) = torch.autograd.grad((pre * g).sum(), d)                         # no activation
    assert float(ref_lin.abs().max()) > 0
    assert torch.allclose(0.5 * ref_lin, linear_dist_grad(g, w, d.detach(), offsets, coeff, scale=0.5), rtol=1e-10,
                          atol=1e-12 * float(ref_lin.abs().max()))


@pytest.mark.parametrize("name", ["MEGNet", "MPNN"])
def test_oracle_forces_match_central_differences_fp64(name):
    """protocol and bound of test_schnet_forces_host.test_oracle_schnet_forces_match_central_differences_fp64 (h = 1e-5, 1e-5
    relative) on the toy batch with self loops and a non-orthogonal cell; dim 16, BatchNorm statistics moved by two optimizer
    steps"""
    pos, node_ptr, cell, pbc, src, tgt, batch = _toy()
    assert (src == tgt).any() and abs(cell[1][1, 0]) > 0
    sh = torch.from_numpy(edge_shifts(pos, node_ptr, cell, pbc, src, tgt))
    s, t = torch.from_numpy(src), torch.from_numpy(tgt)
    torch.manual_seed(5)
    model = getattr(omodels, name)(DS(), dim1=16, dim2=16, dim3=16, gc_count=3, post_fc_count=1).double()
    x = torch.rand(pos.shape[0], 20, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    u = torch.zeros(3, 3, dtype=torch.float64)
    lo, hi = 0.0, 8.0

    def batch_of(p):
        d = edge_dist(p, sh, s, t)
        return types.SimpleNamespace(x=x, edge_index=torch.stack([s, t]), edge_weight=d, u=u,
                                     edge_attr=oops.rbf_expand((d - lo) / (hi - lo), 0.0, 1.0, 16), batch=torch.from_numpy(batch), num_graphs=3)

    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    model.train()
    y = torch.randn(3, dtype=torch.float64, generator=torch.Generator().manual_seed(7))
    for _ in range(2):
        opt.zero_grad()
        torch.nn.functional.l1_loss(model(batch_of(torch.from_numpy(pos))), y).backward()
        opt.step()
    model.eval()
    bns = [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm1d)]
    assert bns and all(float(bn.running_mean.abs().max()) > 0 for bn in bns)

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


def test_new_entry_points_are_declared_and_exported():
    from matdeeplearn_amd import _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mdl_hip.h")).read()
    names = ("mdl_linear_rbf_dist_grad", "mdl_linear_rbf_dist_grad_supported")
    for name in names:
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\b%s\(" % name, header), name
    assert len(_lib.PROTOTYPES["mdl_linear_rbf_dist_grad"][1]) == 16
    handle = _lib.lib()
    for name in names:
        assert hasattr(handle, name), "declared in mdl_hip.h but not exported: " + name
    assert handle.mdl_version() == 100
    for M, G, dt, want in ((1, 1, _lib.MDL_F32, 1), (256, 64, _lib.MDL_BF16, 1), (100, 50, _lib.MDL_F32, 1), (257, 50, _lib.MDL_F32, 0),
                           (64, 65, _lib.MDL_BF16, 0), (0, 50, _lib.MDL_F32, 0), (64, 50, 7, 0)):
        assert handle.mdl_linear_rbf_dist_grad_supported(M, G, dt) == want, (M, G, dt)
    # argument checks come before any launch: they answer without a device
    assert handle.mdl_linear_rbf_dist_grad(None, 64, None, 0, None, _lib.MDL_F32, None, None, -1.0, 1.0, None, 0, 0, 64, 50, None) == 0
    assert handle.mdl_linear_rbf_dist_grad(None, 64, None, 0, None, _lib.MDL_F32, None, None, -1.0, 1.0, None, 0, 5, 300, 50, None) == -2
    assert handle.mdl_linear_rbf_dist_grad(None, 32, None, 0, None, _lib.MDL_F32, None, None, -1.0, 1.0, None, 0, 5, 64, 50, None) == -1
    assert handle.mdl_linear_rbf_dist_grad(None, 64, None, 0, None, _lib.MDL_F32, None, None, -1.0, 1.0, None, 0, 5, 64, 50, None) == -1


def test_gcn_and_other_objects_still_raise_and_the_message_names_all_four():
    from matdeeplearn_amd import forces, models, ops
    with pytest.raises(ops.MdlError, match="CGCNN and SchNet") as e:
        forces.energy_and_forces(models.GCN(DS(), dim1=16, dim2=16, gc_count=1), [], (0.0, 8.0))
    assert "MEGNet" in str(e.value) and "MPNN" in str(e.value)
    with pytest.raises(ops.MdlError, match="CGCNN"):
        forces.energy_and_forces(torch.nn.Linear(2, 2), [], (0.0, 8.0))
