"""Host checks of the stress path's REFERENCE and of its public surface.  The strain gradient the device computes is
dE/d eps_ab (graph b) = sum_{e in b} g_e d_e u_e,a u_e,b  with g_e = dE/dd_e (strain_formula below, fp64); here that formula is pinned
against autograd w.r.t. a zero strain tensor, against central differences of an fp64 oracle CGCNN whose positions AND cell are
really strained, and against the virial of the forces for structures without a cell.  tests/test_gpu_stress.py leans on the same
formula and on the same way of putting eps into the geometry helper (strained).  No GPU."""
import inspect
import os
import re
import types

import numpy as np
import pytest
import torch

from oracle import models as omodels
from oracle import ops as oops
from test_forces_host import DS
from test_gpu_forces import _mixed_structures, _pack, edge_dist, edge_shifts


def strain_formula(g, d, u, graph_of_edge, B):
    """[B, 3, 3] fp64: sum over the edges of every graph of g d u (x) u"""
    t = (g.double() * d.double()).view(-1, 1, 1) * (u.double().unsqueeze(2) * u.double().unsqueeze(1))
    return torch.zeros(B, 3, 3, dtype=torch.float64).index_add_(0, graph_of_edge, t)


def unit_vectors(pos, shift, src, tgt):
    """(d, u) of v = p_tgt + shift - p_src in fp64; u = 0 where d = 0"""
    v = pos.index_select(0, tgt) + shift - pos.index_select(0, src)
    d = v.norm(dim=1)
    return d, torch.where(d.unsqueeze(1) > 0, v / d.clamp_min(1e-300).unsqueeze(1), torch.zeros_like(v))


def strained(pos, shift, eps, graph_of_node, graph_of_edge):
    """positions and image shifts under the homogeneous strain eps [B, 3, 3] of their structure: r -> (I + eps_b) r, so that every
    edge displacement becomes v' = v (I + eps_b)^T"""
    m = torch.eye(3, dtype=eps.dtype) + eps
    return (torch.einsum("nab,nb->na", m[graph_of_node], pos), torch.einsum("eab,eb->ea", m[graph_of_edge], shift))


def all_pairs(node_ptr):
    """every ordered pair inside a structure and the self loops, CSR by target"""
    src, tgt = [], []
    for k in range(len(node_ptr) - 1):
        n = int(node_ptr[k + 1] - node_ptr[k])
        for t in range(n):
            src += [node_ptr[k] + s for s in range(n)]
            tgt += [node_ptr[k] + t] * n
    return np.asarray(src, dtype=np.int64), np.asarray(tgt, dtype=np.int64)


def _mixed_geometry():
    p = _pack(_mixed_structures())
    src, tgt = all_pairs(p["node_ptr"])
    sh = torch.from_numpy(edge_shifts(p["pos"], p["node_ptr"], p["cell"], p["pbc"], src, tgt))
    B = len(p["node_ptr"]) - 1
    gn = torch.from_numpy(np.repeat(np.arange(B), np.diff(p["node_ptr"])))
    s, t = torch.from_numpy(src), torch.from_numpy(tgt)
    return p, torch.from_numpy(p["pos"]), sh, s, t, gn, gn[s], B


def test_formula_matches_autograd_of_a_zero_strain_fp64():
    p, pos, sh, s, t, gn, ge, B = _mixed_geometry()
    w = torch.randn(s.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    eps = torch.zeros(B, 3, 3, dtype=torch.float64, requires_grad=True)
    d = edge_dist(*strained(pos, sh, eps, gn, ge), s, t)
    (auto,) = torch.autograd.grad((d * w).sum(), eps)
    d0, u0 = unit_vectors(pos, sh, s, t)
    assert int((d0 == 0).sum()) == pos.shape[0] + 2                 # the self loops and the coincident pair, both directions
    ref = strain_formula(w, d0, u0, ge, B)
    scale = float(auto.abs().max())
    assert scale > 0 and float((ref - auto).abs().max()) <= 1e-10 * scale
    assert torch.equal(ref, ref.transpose(1, 2))
    assert float(ref[72].abs().max()) == 0.0                        # the one-atom structure: self loop only


def _periodic_toy():
    rng = np.random.default_rng(11)
    sizes = [5, 7, 4, 6]
    node_ptr = np.concatenate([[0], np.cumsum(sizes)])
    cell = np.stack([np.diag([6.0, 7.0, 8.0]), np.array([[6.5, 0, 0], [1.0, 6.0, 0], [0.5, 0.7, 7.0]]), np.eye(3) * 5.5,
                     np.array([[7.0, 0.3, 0], [0, 6.2, 0.4], [-0.8, 0, 6.6]])])
    pbc = np.array([7, 7, 7, 7], dtype=np.int32)
    pos = np.concatenate([rng.uniform(0, 1, (n, 3)) @ cell[k] for k, n in enumerate(sizes)])
    src, tgt = all_pairs(node_ptr)
    return pos, node_ptr, cell, pbc, src, tgt, np.repeat(np.arange(len(sizes)), sizes)


def test_formula_matches_central_differences_of_a_really_strained_crystal_fp64():
    """protocol and bound of test_forces_host.test_oracle_forces_match_central_differences_fp64 (h = 1e-5, 1e-5 of the scale), the
    perturbed variable being one component of the strain of one structure: positions and cell are deformed, the images recomputed"""
    pos, node_ptr, cell, pbc, src, tgt, batch = _periodic_toy()
    B = len(node_ptr) - 1
    sh0 = edge_shifts(pos, node_ptr, cell, pbc, src, tgt)
    s, t = torch.from_numpy(src), torch.from_numpy(tgt)
    ge = torch.from_numpy(batch)[s]
    torch.manual_seed(5)
    model = omodels.CGCNN(DS(), dim1=16, dim2=16, gc_count=3, post_fc_count=1).double()
    with torch.no_grad():
        for bn in model.bn_list:
            bn.running_mean.uniform_(-0.2, 0.2)
            bn.running_var.uniform_(0.5, 1.5)
    model.eval()
    x = torch.rand(pos.shape[0], 20, dtype=torch.float64, generator=torch.Generator().manual_seed(1))
    lo, hi = 0.0, 8.0

    def energy_of(d):
        data = types.SimpleNamespace(x=x, edge_index=torch.stack([s, t]), edge_attr=oops.rbf_expand((d - lo) / (hi - lo), 0.0, 1.0, 16),
                                     batch=torch.from_numpy(batch), num_graphs=B)
        return model(data).sum()

    d0 = edge_dist(torch.from_numpy(pos), torch.from_numpy(sh0), s, t).requires_grad_(True)
    (g,) = torch.autograd.grad(energy_of(d0), d0)
    _, u0 = unit_vectors(torch.from_numpy(pos), torch.from_numpy(sh0), s, t)
    ref = strain_formula(g, d0.detach(), u0, ge, B).numpy()

    def strained_energy(b, i, j, h):
        m = np.tile(np.eye(3), (B, 1, 1))
        m[b, i, j] += h
        pos_s = np.einsum("nab,nb->na", m[batch], pos)
        cell_s = np.einsum("gkb,gab->gka", cell, m)                # every lattice vector (a row) deformed like a position
        sh_s = edge_shifts(pos_s, node_ptr, cell_s, pbc, src, tgt)
        assert np.abs(sh_s - np.einsum("eab,eb->ea", m[ge.numpy()], sh0)).max() <= 1e-12        # the images did not move
        with torch.no_grad():
            return float(energy_of(edge_dist(torch.from_numpy(pos_s), torch.from_numpy(sh_s), s, t)))

    h, fd = 1e-5, np.zeros((B, 3, 3))
    for b in range(B):
        for i in range(3):
            for j in range(3):
                fd[b, i, j] = (strained_energy(b, i, j, h) - strained_energy(b, i, j, -h)) / (2 * h)
    scale = np.abs(fd).max()
    assert scale > 0
    assert np.abs(ref - fd).max() <= 1e-5 * scale, (np.abs(ref - fd).max(), scale)


def test_molecules_strain_gradient_is_the_virial_of_the_forces_fp64():
    p, pos, sh, s, t, gn, ge, B = _mixed_geometry()
    w = torch.randn(s.numel(), dtype=torch.float64, generator=torch.Generator().manual_seed(2))
    pg = pos.clone().requires_grad_(True)
    d = edge_dist(pg, sh, s, t)
    dg = d.detach().requires_grad_(True)
    (g,) = torch.autograd.grad((torch.sin(dg) * w).sum(), dg)
    (gpos,) = torch.autograd.grad((torch.sin(d) * w).sum(), pg)
    d0, u0 = unit_vectors(pos, sh, s, t)
    ref = strain_formula(g, d0, u0, ge, B)
    virial = torch.zeros(B, 3, 3, dtype=torch.float64).index_add_(0, gn, -(pos.unsqueeze(2) * (-gpos).unsqueeze(1)))   # -sum r (x) F
    mol = [b for b in range(B) if int(p["pbc"][b]) == 0]
    assert len(mol) == 18
    scale = float(ref[mol].abs().max())
    assert scale > 0 and float((ref[mol] - virial[mol]).abs().max()) <= 1e-10 * scale


# ---------------------------------------------------------------------------------------------
# surface
# ---------------------------------------------------------------------------------------------
def test_strain_entry_point_is_declared_in_table_header_and_library():
    from matdeeplearn_amd import _build, _lib
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mdl_hip.h")).read()
    for name in ("mdl_edge_strain_grad", "mdl_edge_strain_grad_workspace_bytes"):
        assert name in _lib.PROTOTYPES, name
        assert re.search(r"\b%s\(" % name, header), name
        if os.path.exists(_build.LIB):
            assert hasattr(_lib.lib(), name), name


def test_energy_forces_stress_exists_and_refuses_what_energy_and_forces_refuses():
    from matdeeplearn_amd import forces, models, ops
    for fn in (forces.energy_and_forces, forces.energy_forces_stress):
        with pytest.raises(ops.MdlError) as e:
            fn(models.GCN(DS(), dim1=16, dim2=16, gc_count=1), [], (0.0, 8.0))
        assert "CGCNN and SchNet, MEGNet and MPNN" in str(e.value) and "GCN" in str(e.value)
        with pytest.raises(ops.MdlError, match="on a HIP device"):
            fn(models.CGCNN(DS(), dim1=16, dim2=16, gc_count=1, post_fc_count=1), [], (0.0, 8.0))
    sig = inspect.signature(forces.energy_forces_stress)
    assert list(sig.parameters) == ["model", "structs", "dist_range", "radius", "max_neighbors", "dictionary", "output_index", "fused",
                                    "routes", "volume_normalised"]
    assert sig.parameters["volume_normalised"].default is True


def test_energy_and_forces_signature_is_unchanged():
    from matdeeplearn_amd import forces
    assert str(inspect.signature(forces.energy_and_forces)) == (
        "(model, structs, dist_range, radius=8.0, max_neighbors=12, dictionary=None, output_index=None, fused=True, "
        "routes=('expansion', 'cutoff'))")
