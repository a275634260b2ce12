"""GPU checks of the stress path: the strain-gradient reduction of csrc/edge_geom.hip (ops.edge_strain_grad) against the fp64
formula on the same fp32 operands, and forces.energy_forces_stress for CGCNN, SchNet, MEGNet and MPNN against the fp64 CPU oracle
under autograd w.r.t. a zero strain tensor (each force file's own oracle batch, with the strain put into the geometry helper).
tests/test_stress_host.py pins that formula and that reference against each other and against central differences of a really
strained crystal."""
import copy
import functools
import types

import numpy as np
import pytest
import torch

import test_gpu_forces as tgf
import test_gpu_megnet_mpnn_forces as tgm
import test_gpu_schnet_forces as tgs
from oracle import ops as oops
from test_gpu_forces import DIST_RANGE, DS, F32_TOL, close, dev, edge_dist
from test_stress_host import strain_formula, strained

pytestmark = pytest.mark.gpu


# ---------------------------------------------------------------------------------------------
# 1. the kernel against the fp64 formula on its own fp32 operands
# ---------------------------------------------------------------------------------------------
def _bits_symmetric(t):
    return torch.equal(t.view(torch.int32), t.transpose(1, 2).contiguous().view(torch.int32))


def test_kernel_matches_the_fp64_formula_in_every_variant():
    """74 mixed structures (triclinic cells, slabs, molecules, the one-atom graph, the coincident pair) + one of 60 atoms + two
    coincident atoms alone in a wide cell + an empty graph put into node_ptr; random g.  Bound: the project's fp32 kernel bound
    (the sums are fp64, the result is rounded to fp32 once)."""
    from matdeeplearn_amd import ops
    far = {"positions": np.full((2, 3), 1.5), "numbers": [3, 9], "cell": np.eye(3) * 20.0, "pbc": [True] * 3}
    structs = tgf._mixed_structures() + tgf._bulk_structures(1, seed=5, lo=60, hi=60) + [far]
    p = tgf._pack(structs)
    t, _, _, _, dist_b, _, src, tgt = tgf._graphs(p)
    N, E = p["pos"].shape[0], src.numel()
    dist, u = ops.edge_vectors(t["pos"], t["node_ptr"], t["cell"], t["pbc"], src, tgt, return_unit=True)
    assert torch.equal(dist, dist_b)
    at = 10
    node_ptr = np.insert(p["node_ptr"], at, p["node_ptr"][at])         # graph `at` is empty, the later ones move up by one
    G = len(node_ptr) - 1
    one_atom, pair_only = 72 + 1, 75 + 1
    assert G == 77 and node_ptr[one_atom + 1] - node_ptr[one_atom] == 1 and node_ptr[pair_only + 1] - node_ptr[pair_only] == 2
    ge = torch.from_numpy(np.searchsorted(node_ptr, tgt.cpu().numpy(), side="right") - 1)
    assert int((ge == pair_only).sum()) >= 2 and float(dist[ge.to(dev()) == pair_only].abs().max()) == 0.0
    g = torch.randn(E, generator=torch.Generator().manual_seed(3)).to(dev())
    ref = strain_formula(g.cpu(), dist.cpu(), u.cpu(), ge, G)
    npd = torch.from_numpy(node_ptr).to(dev())
    csr = ops.EdgeCSR(ops.csr_rowptr(tgt, N), src, tgt, None, N, E)
    perm = torch.randperm(E, generator=torch.Generator().manual_seed(4)).to(dev())
    gp, dp, up, sp, tp = g[perm].contiguous(), dist[perm].contiguous(), u[perm].contiguous(), src[perm].contiguous(), tgt[perm].contiguous()
    results = {}
    for slices in (None, 1, 3, 4096):
        results["sorted", slices] = (lambda s=slices: ops.edge_strain_grad(g, dist, u, npd, csr=csr, _slices=s))
        results["permuted", slices] = (lambda s=slices: ops.edge_strain_grad(gp, dp, up, npd, src=sp, tgt=tp, _slices=s))
    assert ops.build_csr(torch.stack([sp, tp]), N).eperm is not None
    outs = {}
    for key, fn in results.items():
        a, b = fn(), fn()
        assert a.dtype == torch.float32 and tuple(a.shape) == (G, 3, 3)
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), key          # no atomics: the same bits outside deterministic mode
        assert _bits_symmetric(a), key
        close(a, ref, *F32_TOL, what="strain gradient %s" % (key,))
        for zero in (at, one_atom, pair_only):
            assert float(a[zero].abs().max()) == 0.0, (key, zero)
        outs[key] = a
    first = outs["sorted", None]
    for key, a in outs.items():
        close(a, first, *F32_TOL, what="%s vs sorted" % (key,))
    assert torch.equal(outs["sorted", None], outs["sorted", 1])                     # a batch of small graphs: one slice
    with ops.deterministic():
        assert torch.equal(ops.edge_strain_grad(g, dist, u, npd, csr=csr), first)


def test_kernel_single_graph_default_split_no_edges_and_bad_arguments():
    from matdeeplearn_amd import ops
    d_ = dev()
    gen = torch.Generator().manual_seed(8)
    N, E = 97, 10001                                                   # one graph, E / G > 4096: sliced by default (5 slices)
    tgt = torch.sort(torch.randint(0, N, (E,), generator=gen)).values.to(torch.int32)
    src = torch.randint(0, N, (E,), generator=gen).to(torch.int32)
    u = torch.nn.functional.normalize(torch.randn(E, 3, generator=gen), dim=1)
    dist, g = torch.rand(E, generator=gen) * 8.0, torch.randn(E, generator=gen)
    ref = strain_formula(g, dist, u, torch.zeros(E, dtype=torch.int64), 1)
    node_ptr = torch.tensor([0, N], device=d_)
    csr = ops.EdgeCSR(ops.csr_rowptr(tgt.to(d_), N), src.to(d_), tgt.to(d_), None, N, E)
    a = ops.edge_strain_grad(g.to(d_), dist.to(d_), u.to(d_), node_ptr, csr=csr)
    b = ops.edge_strain_grad(g.to(d_), dist.to(d_), u.to(d_), node_ptr, csr=csr, _slices=1)
    c = ops.edge_strain_grad(g.to(d_), dist.to(d_), u.to(d_), node_ptr, csr=csr, _slices=5)
    assert tuple(a.shape) == (1, 3, 3) and _bits_symmetric(a) and _bits_symmetric(b)
    close(a, ref, *F32_TOL, what="G = 1, default split")
    close(b, ref, *F32_TOL, what="G = 1, one slice")
    assert torch.equal(a, c)
    assert torch.equal(a, ops.edge_strain_grad(g.to(d_), dist.to(d_), u.to(d_), node_ptr, csr=csr))
    # E = 0
    e32 = torch.zeros(0, dtype=torch.int32, device=d_)
    csr0 = ops.EdgeCSR(ops.csr_rowptr(e32, 5), e32, e32, None, 5, 0)
    np0 = torch.tensor([0, 2, 5], device=d_)
    for slices in (None, 7):
        z = ops.edge_strain_grad(torch.zeros(0, device=d_), torch.zeros(0, device=d_), torch.zeros(0, 3, device=d_), np0, csr=csr0, _slices=slices)
        assert tuple(z.shape) == (2, 3, 3) and float(z.abs().max()) == 0.0
    with pytest.raises(ops.MdlError):
        ops.edge_strain_grad(g.to(d_), dist.to(d_).double(), u.to(d_), node_ptr, csr=csr)
    with pytest.raises(ops.MdlError):
        ops.edge_strain_grad(g.to(d_)[:-1], dist.to(d_), u.to(d_), node_ptr, csr=csr)
    with pytest.raises(ops.MdlError):
        ops.edge_strain_grad(g.to(d_), dist.to(d_), u.to(d_), node_ptr)
    with pytest.raises(ops.MdlError):
        ops.edge_strain_grad(g, dist, u, node_ptr.cpu(), csr=csr)


# ---------------------------------------------------------------------------------------------
# 2. end to end
# ---------------------------------------------------------------------------------------------
def _cgcnn_data(p, x, s, tg, sh, batch, pos):
    """the batch of test_gpu_forces._oracle_forces"""
    d = edge_dist(pos, sh, s, tg)
    return types.SimpleNamespace(x=x.double(), edge_index=torch.stack([s, tg]),
                                 edge_attr=oops.rbf_expand((d - DIST_RANGE[0]) / (DIST_RANGE[1] - DIST_RANGE[0])), batch=batch,
                                 num_graphs=len(p["node_ptr"]) - 1)


def _oracle_strain(m, p, ref_in, data_fn, **kw):
    """the oracle force function of the model's test file with eps added: dE/d eps [B, 3, 3] fp64 at eps = 0"""
    x, s, tg, sh, batch = ref_in
    eps = torch.zeros(len(p["node_ptr"]) - 1, 3, 3, dtype=torch.float64, requires_grad=True)
    pos_s, sh_s = strained(torch.from_numpy(p["pos"]), sh, eps, batch, batch[s])
    pred = m(data_fn(p, x, s, tg, sh_s, batch, pos_s, **kw))
    (g,) = torch.autograd.grad(pred.sum(), eps)
    return g.double()


@functools.lru_cache(maxsize=None)
def _case(name, compute_dtype="fp32"):
    """(structs, p, ref_in, product model, fp32 oracle, fp64 oracle, data_fn, fp64 oracle strain gradient): once per model, shared"""
    if name in ("megnet64", "mpnn64"):
        structs, p, ref_in, ref, m64, _, _ = tgm._setup(name, False)
        model, data_fn = tgm._product(name, ref, compute_dtype), tgm._oracle_data
    else:
        structs = tgf._bulk_structures()
        p = tgf._pack(structs)
        ref_in = tgf._reference_inputs(p)
        if name == "cgcnn64":
            (model, m64), ref, data_fn = tgf._trained_models(64, p, *ref_in), None, _cgcnn_data
        else:
            (model, m64, ref), data_fn = tgs._trained(64, p, ref_in, compute_dtype=compute_dtype), tgs._oracle_data
    return structs, p, ref_in, model, ref, m64, data_fn, _oracle_strain(m64, p, ref_in, data_fn)


@pytest.mark.parametrize("name", ["cgcnn64", "schnet64", "megnet64", "mpnn64"])
def test_energy_forces_stress_matches_the_fp64_oracle(name):
    """dE/d eps (volume_normalised=False) against the fp64 oracle's autograd strain gradient: the force bound, 1e-4 of the batch
    maximum (the same g = dE/dd feeds the force sum and the strain sum).  Measured on an MI355X (error / max|dE/d eps|):
    CGCNN 1.1e-7, SchNet 3.4e-7, MEGNet 1.5e-7, MPNN 5.5e-7 ('Strain gradient')."""
    from matdeeplearn_amd import forces, ops
    structs, p, ref_in, model, _, m64, data_fn, s64 = _case(name)
    B = len(structs)
    with ops.deterministic():                                          # bitwise statements between calls need the repeatable shape
        pred0, f0, node_ptr0 = forces.energy_and_forces(model, structs, DIST_RANGE)
        pred, f, strain, node_ptr = forces.energy_forces_stress(model, structs, DIST_RANGE, volume_normalised=False)
        pred_n, f_n, stress, _ = forces.energy_forces_stress(model, p, DIST_RANGE)
    assert strain.dtype == torch.float32 and tuple(strain.shape) == (B, 3, 3) and _bits_symmetric(strain)
    assert torch.equal(pred, pred0) and torch.equal(f, f0) and torch.equal(node_ptr, node_ptr0)
    assert torch.equal(pred_n, pred0) and torch.equal(f_n, f0)
    scale = float(s64.abs().max())
    err = float((strain.double().cpu() - s64).abs().max())
    print("%s: max|dE/d eps| %.3e, strain gradient error %.3e (%.2e of the maximum; bound 1e-4)" % (name, scale, err, err / scale))
    assert torch.allclose(strain.double().cpu(), s64, rtol=1e-4, atol=1e-4 * scale), "%s: strain gradient error %.3e (max %.3e)" % (name, err, scale)
    vol = np.abs(np.linalg.det(p["cell"]))
    assert torch.isfinite(stress).all() and _bits_symmetric(stress)
    assert torch.allclose(stress.double().cpu(), strain.double().cpu() / torch.from_numpy(vol).view(-1, 1, 1), rtol=1e-6, atol=0.0)
    assert all(q.grad is None for q in model.parameters())
    # outside deterministic mode the reduction itself is still repeatable; the whole call meets the same bound
    strain2 = forces.energy_forces_stress(model, structs, DIST_RANGE, volume_normalised=False)[2]
    assert torch.allclose(strain2.double().cpu(), s64, rtol=1e-4, atol=1e-4 * scale)


def test_mixed_structures_rows_without_a_volume_are_nan():
    from matdeeplearn_amd import forces, models
    structs = tgf._mixed_structures()
    torch.manual_seed(0)
    model = models.CGCNN(DS(), dim1=64, dim2=64, gc_count=2, post_fc_count=1).to(dev()).eval()
    _, _, stress, _ = forces.energy_forces_stress(model, structs, DIST_RANGE)
    _, _, strain, _ = forces.energy_forces_stress(model, structs, DIST_RANGE, volume_normalised=False)
    no_volume = torch.tensor([not all(s["pbc"]) for s in structs])
    assert int(no_volume.sum()) == 36                                   # the slabs and the molecules
    nan_rows = torch.isnan(stress).view(len(structs), 9).cpu()
    assert torch.equal(nan_rows.all(1), no_volume) and torch.equal(nan_rows.any(1), no_volume)
    assert torch.isfinite(stress[~no_volume.to(dev())]).all() and torch.isfinite(strain).all()
    assert float(strain[no_volume.to(dev())].abs().max()) > 0           # the unnormalised form serves them too
    assert float(strain[72].abs().max()) == 0.0                         # one atom: a self loop only


def test_schnet_routes_add_up_to_the_strain_gradient():
    """the statement test_gpu_schnet_forces makes about forces (shares within 1e-5 of the maximum of the whole)"""
    from matdeeplearn_amd import forces
    structs, p, ref_in, model, _, m64, data_fn, s64 = _case("schnet64")
    scale = float(s64.abs().max())
    full = forces.energy_forces_stress(model, p, DIST_RANGE, volume_normalised=False)[2]
    parts = {}
    for route, kw in (("expansion", dict(cut_route=False)), ("cutoff", dict(exp_route=False))):
        parts[route] = forces.energy_forces_stress(model, p, DIST_RANGE, routes=(route,), volume_normalised=False)[2]
        o = _oracle_strain(m64, p, ref_in, data_fn, **kw)
        err = float((parts[route].double().cpu() - o).abs().max())
        print("%s route: share max %.3e, error %.2e of max|dE/d eps|" % (route, float(o.abs().max()), err / scale))
        assert float((parts[route] - full).abs().max()) > 1e-3 * scale, route
        assert err <= 1e-4 * scale, route
    assert float((parts["expansion"] + parts["cutoff"] - full).abs().max()) <= 1e-5 * scale


def test_bf16_strain_gradient_within_the_oracles_own_sensitivity():
    """protocol of test_gpu_megnet_mpnn_forces.test_bf16_and_split_mode_forces: the bf16 error against the fp64 oracle is reported
    and asserted to be within 4x the oracle's own sensitivity to bf16 storage (fp32 oracle with bf16-rounded weights, node and
    edge features against the fp64 oracle)."""
    from matdeeplearn_amd import forces
    structs, p, ref_in, _, ref, m64, data_fn, s64 = _case("megnet64")
    scale = float(s64.abs().max())
    mr = copy.deepcopy(ref).eval()
    with torch.no_grad():
        for q in mr.parameters():
            if q.dim() == 2:
                q.copy_(q.bfloat16().float())
    rb = lambda t: t + (t.detach().bfloat16().to(t.dtype) - t.detach())
    sens = float((_oracle_strain(mr, p, ref_in, data_fn, dtype=torch.float32, rb=rb) - s64).abs().max()) / scale
    model = tgm._product("megnet64", ref, "bf16")
    strain = forces.energy_forces_stress(model, structs, DIST_RANGE, volume_normalised=False)[2]
    err = float((strain.double().cpu() - s64).abs().max()) / scale
    print("bf16 megnet64: oracle bf16-storage sensitivity %.3e of max|dE/d eps|, strain gradient error %.3e (bound %.3e)" % (sens, err, 4 * sens))
    assert _bits_symmetric(strain) and err <= 4 * sens
