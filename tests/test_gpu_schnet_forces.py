"""GPU checks of SchNet's force path: the CFConv gradients w.r.t. the per-edge inputs (csrc/cfconv_de.hip, both epilogues, and
the scale gradient of the unfused sequence), the general composition for shapes the kernel refuses, and
forces.energy_and_forces(models.SchNet).  Reference: the project's CPU oracle under autograd (oracle.ops / oracle.models are
pure torch) with the geometry helpers of tests/test_gpu_forces.py; tests/test_schnet_forces_host.py pins that reference
against central differences."""
import copy
import math
import types

import numpy as np
import pytest
import torch

import test_gpu_forces as tgf
from oracle import models as omodels
from oracle import ops as oops
from test_gpu_forces import BF16_TOL, DIST_RANGE, DS, F32_TOL, close, dev, edge_dist

pytestmark = pytest.mark.gpu
LN2 = math.log(2.0)


def _inputs(n, F, G, dtype, sort, seed, empty_frac=0.1):
    g = torch.Generator().manual_seed(seed)
    ei = tgf.rand_graph(n, seed, sort=sort, empty_frac=empty_frac)
    E = ei.shape[1]
    rnd = lambda *s: torch.randn(*s, generator=g)
    r = lambda t: t.to(dtype).float()
    dn = torch.rand(E, generator=g)
    cut = torch.rand(E, generator=g)
    h, gout = r(rnd(n, F)), r(rnd(n, F))
    w1, w2 = r(rnd(F, G) * (2.0 / G ** 0.5)), r(rnd(F, F) * (2.0 / F ** 0.5))
    b1, b2 = rnd(F) * 0.1, rnd(F) * 0.1
    return ei, dn, cut, h, gout, w1, b1, w2, b2


def _oracle_agg(rbf, cut, h, ei, w1, b1, w2, b2):
    a = torch.nn.functional.softplus(rbf @ w1.t() + b1) - LN2
    w = (a @ w2.t() + b2) * cut.view(-1, 1)
    return oops.scatter(h.index_select(0, ei[0]) * w, ei[1], 0, h.shape[0], "sum")


def _lins(w1, b1, w2, b2, d):
    la, lb = torch.nn.Linear(w1.shape[1], w1.shape[0]), torch.nn.Linear(w2.shape[1], w2.shape[0])
    with torch.no_grad():
        la.weight.copy_(w1); la.bias.copy_(b1); lb.weight.copy_(w2); lb.bias.copy_(b2)
    return la.to(d), lb.to(d)


# ---------------------------------------------------------------------------------------------
# 1. general epilogue (drbf) and dcut against the oracle under autograd
# ---------------------------------------------------------------------------------------------
def _general_case(n, F, G, dtype, sort, seed, empty_frac=0.1, pad=0):
    from matdeeplearn_amd import ops
    ei, dn, cut, h, gout, w1, b1, w2, b2 = _inputs(n, F, G, dtype, sort, seed, empty_frac)
    rbf = torch.rand(ei.shape[1], G, generator=torch.Generator().manual_seed(seed + 2)).to(dtype).float()
    ro, co, ho = [t.double().clone().requires_grad_(True) for t in (rbf, cut, h)]
    po = [t.double().clone().requires_grad_(True) for t in (w1, b1, w2, b2)]
    ref = _oracle_agg(ro, co, ho, ei, *po)
    (ref * gout.double()).sum().backward()

    d = dev()
    E = ei.shape[1]
    csr = ops.build_csr(ei.to(d), n, assume_sorted=sort)
    rbf_d, cut_d = rbf.to(d).to(dtype), cut.to(d)
    if pad:                                                    # a padded static batch: rows past rowptr[N] belong to no node
        assert sort
        fill = torch.zeros(pad, dtype=torch.int32, device=d)
        csr = ops.EdgeCSR(csr.rowptr, torch.cat([csr.src, fill]), torch.cat([csr.tgt, fill]), None, n, E + pad)
        csr.partial = True
        rbf_d = torch.cat([rbf_d, torch.rand(pad, G, device=d).to(dtype)])
        cut_d = torch.cat([cut_d, torch.rand(pad, device=d)])
    rbf_d.requires_grad_(True)
    cut_d.requires_grad_(True)
    hd = h.to(d).to(dtype).requires_grad_(not pad)
    la, lb = _lins(w1, b1, w2, b2, d)
    if pad:
        for q in list(la.parameters()) + list(lb.parameters()):
            q.requires_grad_(False)
    before = ops.K4D_LAUNCHES["general"]
    out = ops.cfconv(rbf_d, cut_d, hd, csr, la, lb)
    (out.float() * gout.to(d)).sum().backward()
    assert ops.K4D_LAUNCHES["general"] == before + (1 if E else 0)          # the kernel, not the general composition
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    assert rbf_d.grad.dtype == dtype and rbf_d.grad.shape == rbf_d.shape and cut_d.grad.dtype == torch.float32
    close(out, ref, *tol, what="out")
    if E:
        close(rbf_d.grad[:E], ro.grad, *tol, what="drbf")
        close(cut_d.grad[:E], co.grad, *tol, what="dcut")
    if pad:
        assert float(rbf_d.grad[E:].abs().max()) == 0.0 and float(cut_d.grad[E:].abs().max()) == 0.0
        return
    close(hd.grad, ho.grad, *tol, what="dh")
    for name, q, qo in zip(("dW1", "db1", "dW2", "db2"), (la.weight, la.bias, lb.weight, lb.bias), po):
        close(q.grad, qo.grad, *tol, what=name)


@pytest.mark.parametrize("F", [64, 100, 128, 150])
@pytest.mark.parametrize("sort", [True, False])
def test_cfconv_edge_gradients_match_oracle_bf16(F, sort):
    _general_case(200, F, 50, torch.bfloat16, sort, seed=F + 7)


@pytest.mark.parametrize("F", [64, 150])
@pytest.mark.parametrize("sort", [True, False])
def test_cfconv_edge_gradients_match_oracle_fp32(F, sort):
    _general_case(200, F, 50, torch.float32, sort, seed=F + 9)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cfconv_edge_gradients_isolated_nodes_no_edges_padded_batch(dtype):
    from matdeeplearn_amd import ops
    _general_case(150, 64, 50, dtype, True, seed=5, empty_frac=0.5)
    _general_case(130, 150, 50, dtype, True, seed=6, pad=77)
    d = dev()
    ei = torch.zeros(2, 0, dtype=torch.int64, device=d)
    la, lb = _lins(torch.randn(64, 50) * 0.1, torch.zeros(64), torch.randn(64, 64) * 0.1, torch.zeros(64), d)
    rbf = torch.zeros(0, 50, device=d, dtype=dtype, requires_grad=True)
    cut = torch.zeros(0, device=d, requires_grad=True)
    out = ops.cfconv(rbf, cut, torch.randn(5, 64, device=d).to(dtype), ops.build_csr(ei, 5, assume_sorted=True), la, lb)
    out.float().sum().backward()
    assert float(out.abs().max()) == 0.0 and rbf.grad.shape == (0, 50) and cut.grad.shape == (0,)


# ---------------------------------------------------------------------------------------------
# 2. distance epilogue
# ---------------------------------------------------------------------------------------------
def _oracle_dd(dn, cut, h, gout, ei, w1, b1, w2, b2, G, round_bf16=False):
    rb = (lambda t: t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())) if round_bf16 else (lambda t: t)
    dg = dn.clone().requires_grad_(True)
    cg = cut.clone().requires_grad_(True)
    out = _oracle_agg(rb(oops.rbf_expand(dg, 0.0, 1.0, G, 0.2)), cg, rb(h), ei, rb(w1), b1, rb(w2), b2)
    (out * rb(gout)).sum().backward()
    return dg.grad, cg.grad


def _dist_case(n, F, G, dtype, sort, seed):
    from matdeeplearn_amd import ops
    ei, dn, cut, h, gout, w1, b1, w2, b2 = _inputs(n, F, G, torch.float32, sort, seed)
    args = (dn, cut, h, gout, ei, w1, b1, w2, b2)
    ref64, refc64 = _oracle_dd(*[t.double() if t.is_floating_point() else t for t in args], G)
    scale = float(ref64.abs().max())
    if dtype == torch.float32:
        bound = 2e-5
    else:
        sens = float((_oracle_dd(*args, G, round_bf16=True)[0].double() - ref64).abs().max()) / scale
        bound = 4 * sens
        print("F=%d sort=%s: reference sensitivity to bf16 storage %.3e of scale -> bound %.3e" % (F, sort, sens, bound))
    d = dev()
    csr = ops.build_csr(ei.to(d), n, assume_sorted=sort)
    hd, gd = h.to(d).to(dtype), gout.to(d).to(dtype)
    P = [t.to(d) for t in (w1, b1, w2, b2)]
    before = ops.K4D_LAUNCHES["distance"]
    dd, dcut = ops.cfconv_dist_grad(hd, ei.to(d), dn.to(d), cut.to(d), *P, gd, csr=csr, resolution=G, want_dcut=True)
    assert ops.K4D_LAUNCHES["distance"] == before + 1
    assert dd.dtype == torch.float32 and dd.shape == dn.shape
    close(dd, ref64, bound, bound, what="dd")
    close(dcut, refc64, *(F32_TOL if dtype == torch.float32 else BF16_TOL), what="dcut")
    # the autograd route (ops.cfconv(dist=...)): the same launch, the same bits, for d_norm and for the cutoff
    dg, cg = dn.to(d).requires_grad_(True), cut.to(d).requires_grad_(True)
    offs = ops.rbf_offsets(0.0, 1.0, G, d)
    ea = ops.rbf_expand(dg.detach(), 0.0, 1.0, G, 0.2, out_dtype=dtype, offsets=offs)
    la, lb = _lins(w1, b1, w2, b2, d)
    out = ops.cfconv(ea, cg, hd, csr, la, lb, dist=(dg, offs, ops.rbf_coeff(0.0, 1.0, 0.2)))
    g1, g2 = torch.autograd.grad((out.float() * gd.float()).sum(), [dg, cg])
    assert torch.equal(g1, dd) and torch.equal(g2, dcut)
    if sort:                                                   # two calls accumulate in one buffer; scale is applied
        buf = torch.zeros_like(dd)
        for _ in range(2):
            ops.cfconv_dist_grad(hd, ei.to(d), dn.to(d), cut.to(d), *P, gd, csr=csr, resolution=G, scale=0.5, out=buf)
        close(buf, dd, 1e-6, 1e-6, what="two half-scaled calls")
    again = ops.cfconv_dist_grad(hd, ei.to(d), dn.to(d), cut.to(d), *P, gd, csr=csr, resolution=G)
    assert torch.equal(again, dd)                              # bitwise repeatable


@pytest.mark.parametrize("n,F,sort", [(200, 64, True), (200, 150, False), (900, 150, True), (130, 100, False)])
def test_cfconv_distance_epilogue_matches_oracle_fp32(n, F, sort):
    """dL/dd_norm of one CFConv aggregation against the fp64 oracle: 2e-5 of the scale (the project's fp32 kernel bound)."""
    _dist_case(n, F, 50, torch.float32, sort, seed=n + F)


@pytest.mark.parametrize("n,F,sort", [(200, 64, True), (200, 100, False), (200, 128, True), (300, 150, False)])
def test_cfconv_distance_epilogue_bf16_within_the_references_own_sensitivity(n, F, sort):
    """bf16 has no pre-set bound: per case the reference's own sensitivity to the storage rounding (fp32 oracle on bf16-rounded
    rbf, h, g and weights against the fp64 oracle on the unrounded values) is measured and the kernel, which also rounds a_e,
    W_e, c q and da to bf16, is allowed 4x that.  Sensitivity and kernel error per case are printed."""
    _dist_case(n, F, 50, torch.bfloat16, sort, seed=n + F)


# ---------------------------------------------------------------------------------------------
# 3. the scale gradient of the unfused sequence
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("with_w", [True, False])
def test_edge_dot_and_gather_mul_reduce_scale_gradient(dtype, with_w):
    from matdeeplearn_amd import _lib, ops
    n, F = 120, 150
    ei, _, cut, h, gout, *_ = _inputs(n, F, 50, dtype, False, 21)            # permuted edge order
    E = ei.shape[1]
    w = torch.randn(E, F, generator=torch.Generator().manual_seed(4)).to(dtype).float() if with_w else None
    d = dev()
    hd, gd = h.to(d).to(dtype), gout.to(d).to(dtype)
    wd = None if w is None else w.to(d).to(dtype)
    src32, tgt32 = ei[0].to(d).to(torch.int32), ei[1].to(d).to(torch.int32)
    out = torch.empty(E, device=d)
    _lib.check(_lib.lib().mdl_edge_dot(_lib.ptr(gd), _lib.ptr(tgt32), _lib.ptr(hd), _lib.ptr(src32), _lib.ptr(wd), _lib.ptr(out), E, F,
                                       _lib.dtype_code(hd), _lib.stream()), "mdl_edge_dot")
    gs, hs = gout.double()[ei[1]], h.double()[ei[0]]
    ref = torch.einsum("ef,ef->e", gs * hs, torch.ones_like(gs) if w is None else w.double())
    close(out, ref, 2e-5, 2e-5, what="edge_dot")               # fp32 sums of exact inputs in both dtypes
    # ops.gather_mul_reduce(scale=c) with c.requires_grad
    csr = ops.build_csr(ei.to(d), n)
    c = cut.to(d).requires_grad_(True)
    hq = hd.clone().requires_grad_(True)
    wq = None if wd is None else wd.clone().requires_grad_(True)
    o = ops.gather_mul_reduce(hq, csr, w=wq, scale=c, reduce="sum")
    (o.float() * gd.float()).sum().backward()
    close(c.grad, ref, 2e-5, 2e-5, what="dscale")
    co, ho = cut.double().requires_grad_(True), h.double().requires_grad_(True)
    msg = ho[ei[0]] * co.view(-1, 1) * (1.0 if w is None else w.double())
    (oops.scatter(msg, ei[1], 0, n, "sum") * gout.double()).sum().backward()
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    close(c.grad, co.grad, *tol, what="dscale vs autograd")
    close(hq.grad, ho.grad, *tol, what="dh")


# ---------------------------------------------------------------------------------------------
# 4. shapes K4d refuses: the general composition
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F,G", [(64, 32), (40, 50)])
def test_refused_shapes_take_the_general_composition_bf16(F, G):
    from matdeeplearn_amd import _lib, nn as mnn, ops
    assert not _lib.lib().mdl_cfconv_bwd_edge_supported(F, G, _lib.MDL_BF16)
    n, C, cutoff = 150, 64, 8.0
    g = torch.Generator().manual_seed(F + G)
    ei = tgf.rand_graph(n, 3, sort=True)
    E = ei.shape[1]
    torch.manual_seed(F)
    ref = oops.InteractionBlock(C, G, F, cutoff)
    blk = mnn.InteractionBlock(C, G, F, cutoff)
    blk.load_state_dict(ref.state_dict())
    blk.to(dev())
    x = torch.randn(n, C, generator=g).bfloat16().float()
    ea = torch.rand(E, G, generator=g).bfloat16().float()
    dist = torch.rand(E, generator=g) * 7.5
    gout = torch.randn(n, F, generator=g).bfloat16().float()
    eo, do = ea.double().requires_grad_(True), dist.double().requires_grad_(True)
    r64 = copy.deepcopy(ref).double()
    c64 = 0.5 * (torch.cos(do * math.pi / cutoff) + 1.0)
    agg = oops.scatter(r64.conv.lin1(x.double()).index_select(0, ei[0]) * r64.mlp(eo) * c64.view(-1, 1), ei[1], 0, n, "sum")
    (agg * gout.double()).sum().backward()
    d = dev()
    ed, dd_ = ea.to(d).bfloat16().requires_grad_(True), dist.to(d).requires_grad_(True)
    before = sum(ops.K4D_LAUNCHES.values())
    out = blk.conv.aggregate(x.to(d).bfloat16(), None, dd_, ed, csr=ops.build_csr(ei.to(d), n, assume_sorted=True))
    (out.float() * gout.to(d)).sum().backward()
    assert sum(ops.K4D_LAUNCHES.values()) == before
    close(out, agg, *BF16_TOL, what="agg")
    close(ed.grad, eo.grad, *BF16_TOL, what="d edge_attr")
    close(dd_.grad, do.grad, *BF16_TOL, what="d distance (cutoff route)")


# ---------------------------------------------------------------------------------------------
# 5. / 6. end to end
# ---------------------------------------------------------------------------------------------
def _oracle_data(p, x, s, tg, sh, batch, pos, dtype=torch.float64, cut_route=True, exp_route=True, rb=lambda t: t):
    d = edge_dist(pos, sh, s, tg).to(dtype)
    dn = (d - DIST_RANGE[0]) / (DIST_RANGE[1] - DIST_RANGE[0])
    return types.SimpleNamespace(x=rb(x.to(dtype)), edge_index=torch.stack([s, tg]), edge_weight=d if cut_route else d.detach(),
                                 edge_attr=rb(oops.rbf_expand(dn if exp_route else dn.detach())), batch=batch,
                                 num_graphs=len(p["node_ptr"]) - 1)


def _oracle_forces(m, p, ref_in, **kw):
    pos = torch.from_numpy(p["pos"]).requires_grad_(True)
    pred = m(_oracle_data(p, *ref_in, pos, **kw))
    (g,) = torch.autograd.grad(pred.sum(), pos)
    return pred.detach().double(), -g


def _trained(dim, p, ref_in, compute_dtype="fp32"):
    from matdeeplearn_amd import models
    torch.manual_seed(0)
    kw = dict(dim1=dim, dim2=dim, dim3=dim, gc_count=3, post_fc_count=1)
    ref = omodels.SchNet(DS(), **kw)
    data = _oracle_data(p, *ref_in, torch.from_numpy(p["pos"]), dtype=torch.float32)
    y = torch.randn(data.num_graphs, generator=torch.Generator().manual_seed(7))
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    ref.train()
    for _ in range(2):
        opt.zero_grad()
        torch.nn.functional.l1_loss(ref(data), y).backward()
        opt.step()
    ref.eval()
    model = models.SchNet(DS(), compute_dtype=compute_dtype, **kw)
    model.load_state_dict(ref.state_dict())
    return model.to(dev()).eval(), copy.deepcopy(ref).double().eval(), ref


def _check(f, pred, f64, pred64, what, tol=1e-4):
    scale = float(f64.abs().max())
    ferr = float((f.double().cpu() - f64).abs().max())
    perr = float((pred.double().cpu() - pred64).abs().max()) / float(pred64.abs().max())
    print("%s: max|F| %.3e, force error %.2e of max|F|, prediction error %.2e of max (bound %.1e)" % (what, scale, ferr / scale, perr, tol))
    assert torch.allclose(pred.double().cpu(), pred64, rtol=tol, atol=tol * float(pred64.abs().max())), what
    assert torch.allclose(f.double().cpu(), f64, rtol=tol, atol=tol * scale), "%s: force error %.3e (max|F| %.3e)" % (what, ferr, scale)


@pytest.mark.parametrize("dim,mixed", [(64, False), (150, False), (64, True)])
def test_schnet_energy_and_forces_match_the_fp64_oracle(dim, mixed):
    from matdeeplearn_amd import forces, ops
    structs = tgf._mixed_structures() if mixed else tgf._bulk_structures()
    p = tgf._pack(structs)
    ref_in = tgf._reference_inputs(p)
    model, m64, _ = _trained(dim, p, ref_in)
    pred64, f64 = _oracle_forces(m64, p, ref_in)
    before = ops.K4D_LAUNCHES["distance"]
    pred, f, node_ptr = forces.energy_and_forces(model, structs, DIST_RANGE)
    assert ops.K4D_LAUNCHES["distance"] == before + 3
    assert f.dtype == torch.float32 and f.shape == (p["pos"].shape[0], 3) and torch.equal(node_ptr.cpu(), torch.from_numpy(p["node_ptr"]))
    _check(f, pred, f64, pred64, "fused")
    pred_u, f_u, _ = forces.energy_and_forces(model, p, DIST_RANGE, fused=False)
    _check(f_u, pred_u, f64, pred64, "general")
    assert torch.equal(pred_u, pred)
    fn = f.double().cpu()
    for b in range(len(structs)):
        fb = fn[p["node_ptr"][b]:p["node_ptr"][b + 1]]
        assert float(fb.sum(0).norm()) <= 1e-5 * float(fb.norm(dim=1).sum()) + 1e-30, b
    if not mixed:
        moved = [dict(s, positions=s["positions"] + s["cell"][k % 3]) for k, s in enumerate(structs)]
        pred_m, f_m, _ = forces.energy_and_forces(model, moved, DIST_RANGE)
        _check(f_m, pred_m, f64, pred64, "shifted by a lattice vector")
    with ops.deterministic():
        a = forces.energy_and_forces(model, p, DIST_RANGE)[1]
        b = forces.energy_and_forces(model, p, DIST_RANGE)[1]
    assert torch.equal(a, b)
    assert all(q.grad is None for q in model.parameters())

    # 6. the two routes separately: each differs from the full force, each matches the oracle with the same route cut, and
    # the shares add up (what catches a kernel that drops dcut)
    f_exp = forces.energy_and_forces(model, p, DIST_RANGE, routes=("expansion",))[1]
    f_cut = forces.energy_and_forces(model, p, DIST_RANGE, routes=("cutoff",))[1]
    scale = float(f64.abs().max())
    _, o_exp = _oracle_forces(m64, p, ref_in, cut_route=False)
    _, o_cut = _oracle_forces(m64, p, ref_in, exp_route=False)
    for name, part, opart in (("expansion route", f_exp, o_exp), ("cutoff route", f_cut, o_cut)):
        err = float((part.double().cpu() - opart).abs().max())
        print("%s: share max %.3e, error %.2e of max|F|" % (name, float(opart.abs().max()), err / scale))
        assert float((part - f).abs().max()) > 1e-3 * scale, name
        assert err <= 1e-4 * scale, name
    assert float((f_exp + f_cut - f).abs().max()) <= 1e-5 * scale


def test_schnet_bf16_and_split_mode_forces():
    """A bf16 SchNet: the force error against the fp64 oracle is reported and asserted only to be within 4x the oracle's own
    sensitivity to bf16 storage (fp32 oracle with bf16-rounded parameters, node and edge features against the fp64 oracle).  A
    "bf16x3" SchNet runs the exact fp32 form."""
    from matdeeplearn_amd import forces, ops
    structs = tgf._bulk_structures()
    p = tgf._pack(structs)
    ref_in = tgf._reference_inputs(p)
    model, m64, m32 = _trained(64, p, ref_in, compute_dtype="bf16")
    pred64, f64 = _oracle_forces(m64, p, ref_in)
    scale = float(f64.abs().max())
    mr = copy.deepcopy(m32).eval()
    with torch.no_grad():
        for q in mr.parameters():
            if q.dim() == 2:
                q.copy_(q.bfloat16().float())
    rb = lambda t: t + (t.detach().bfloat16().to(t.dtype) - t.detach())
    _, fr = _oracle_forces(mr, p, ref_in, dtype=torch.float32, rb=rb)
    sens = float((fr.double() - f64).abs().max()) / scale
    before = ops.K4D_LAUNCHES["distance"]
    pred, f, _ = forces.energy_and_forces(model, structs, DIST_RANGE)
    assert ops.K4D_LAUNCHES["distance"] == before + 3
    err = float((f.double().cpu() - f64).abs().max()) / scale
    print("bf16 SchNet: oracle bf16-storage sensitivity %.3e of max|F|, force error %.3e of max|F| (bound %.3e)" % (sens, err, 4 * sens))
    assert err <= 4 * sens
    f_u = forces.energy_and_forces(model, structs, DIST_RANGE, fused=False)[1]
    print("bf16 SchNet general route: force error %.3e of max|F|" % (float((f_u.double().cpu() - f64).abs().max()) / scale))
    m3, _, _ = _trained(64, p, ref_in, compute_dtype="bf16x3")
    pred3, f3, _ = forces.energy_and_forces(m3, structs, DIST_RANGE)
    _check(f3, pred3, f64, pred64, "bf16x3 (exact fp32 form)")


def test_other_models_still_raise():
    from matdeeplearn_amd import forces, models, ops
    with pytest.raises(ops.MdlError, match="CGCNN and SchNet"):
        forces.energy_and_forces(models.GCN(DS(), dim1=64, dim2=64, gc_count=1).to(dev()), tgf._bulk_structures(2), DIST_RANGE)


# ---------------------------------------------------------------------------------------------
# 7. nothing else moved
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("F", [128, 64])             # the recomputing path (F >= 96) and the stored-activation path
def test_cfconv_without_edge_gradient_is_what_it_was(F):
    """a bf16 training step through nn.CFConv.aggregate (no gradient on the edge inputs) gives bitwise the loss and gradients of
    the same step through the pre-existing entry points, called here the way aggregate always called them"""
    from matdeeplearn_amd import nn as mnn, ops
    n, C, G = 2000, 64, 50
    g = torch.Generator().manual_seed(F)
    ei = tgf.rand_graph(n, 17, sort=True)
    E = ei.shape[1]
    d = dev()
    torch.manual_seed(F)
    blk = mnn.InteractionBlock(C, G, F, 8.0).to(d)
    x = torch.randn(n, C, generator=g).to(d).bfloat16()
    ea = torch.rand(E, G, generator=g).to(d).bfloat16()
    c = torch.rand(E, generator=g).to(d)
    gout = torch.randn(n, F, generator=g).to(d)
    csr = ops.build_csr(ei.to(d), n, assume_sorted=True)
    conv = blk.conv

    def old(xq):
        h = mnn._lin(conv.lin1, xq)
        mods = list(conv.nn)
        assert ops.cfconv_fused_ok(ea, h, csr, mods[0], mods[2])
        if F >= ops._CFCONV_RECOMPUTE_MIN_F:
            return ops.cfconv_recompute(ea, c, h, csr, mods[0], mods[2], None)
        agg, a1, w = ops.cfconv_fused(ea, c, h.detach(), csr, mods[0], mods[2], want_acts=True)
        w = mnn._seq(conv.nn, ea, pre=[a1, w])
        return ops.gather_mul_reduce(h, csr, w=w, scale=c, reduce="sum", pre=agg)

    def run(fn):
        blk.zero_grad(set_to_none=True)
        xq = x.clone().requires_grad_(True)
        out = fn(xq)
        loss = (out.float() * gout).sum()
        loss.backward()
        return [loss.detach(), out.detach(), xq.grad] + [q.grad.clone() for q in blk.parameters() if q.grad is not None]

    before = sum(ops.K4D_LAUNCHES.values())
    with ops.deterministic():
        a = run(old)
        b = run(lambda xq: conv.aggregate(xq, None, None, ea, csr=csr, cut=c))
    assert sum(ops.K4D_LAUNCHES.values()) == before and len(a) == len(b) >= 8
    for u, v in zip(a, b):
        assert torch.equal(u, v)
