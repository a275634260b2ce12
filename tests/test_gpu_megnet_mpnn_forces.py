"""GPU checks of the MEGNet / MPNN force path: the distance gradient of a dense layer on the Gaussian expansion
(csrc/linear_de.hip) against the fp64 formula, the autograd node ops.rbf_linear_act (same forward, same weight gradients, the
general composition for shapes the kernel refuses) and forces.energy_and_forces(models.MEGNet / models.MPNN).  Reference: the
project's CPU oracle under autograd (oracle.models is pure torch) with the geometry helpers of tests/test_gpu_forces.py;
tests/test_linear_dist_grad_host.py pins the formula against autograd and that reference against central differences."""
import copy
import functools
import types

import pytest
import torch

import test_gpu_forces as tgf
from oracle import models as omodels
from oracle import ops as oops
from test_gpu_forces import BF16_TOL, DIST_RANGE, DS, F32_TOL, close, dev, edge_dist
from test_gpu_schnet_forces import _check
from test_linear_dist_grad_host import linear_dist_grad as formula

pytestmark = pytest.mark.gpu
COEFF = -0.5 / 0.2 ** 2


# ---------------------------------------------------------------------------------------------
# 1. the kernel against the fp64 formula on operands rounded to the storage dtype
# ---------------------------------------------------------------------------------------------
def _operands(E, M, G, dtype, seed, wide=0):
    """g, act_y (ReLU output with planted exact zeros), W rounded to dtype; d fp32.  wide: g and act_y are column slices of
    tensors `wide` columns wider (leading dimension > M, rows that start off the 16-byte grid)"""
    gen = torch.Generator().manual_seed(seed)
    r = lambda t: t.to(dtype)
    g = r(torch.randn(E, M + wide, generator=gen))
    y = r(torch.relu(torch.randn(E, M + wide, generator=gen)))
    y[::3] = 0
    w = r(torch.randn(M, G, generator=gen) * (2.0 / G ** 0.5))
    d = torch.rand(E, generator=gen)
    return g, y, w, d


def _ref(g, y, w, d, G, scale=1.0):
    return formula(g.double(), w.double(), d.double(), oops.rbf_offsets(0.0, 1.0, G).double(), COEFF, None if y is None else y.double(), scale)


@pytest.mark.parametrize("M", [1, 64, 100, 150, 256])
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernel_matches_the_fp64_formula(dtype, M):
    from matdeeplearn_amd import ops
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    d_ = dev()
    for G in (50, 64):
        for E in (1, 63, 64, 65, 1000):
            g, y, w, d = _operands(E, M, G, dtype, seed=E + M + G)
            gd, yd, wd, dd_ = g.to(d_), y.to(d_), w.to(d_), d.to(d_)
            before = ops.LIN_DD_LAUNCHES["distance"]
            out = ops.linear_dist_grad(gd, wd, dd_, resolution=G)
            out_m = ops.linear_dist_grad(gd, wd, dd_, act_y=yd, resolution=G)
            assert ops.LIN_DD_LAUNCHES["distance"] == before + 2
            assert out.dtype == torch.float32 and out.shape == (E,)
            close(out, _ref(g, None, w, d, G), *tol, what="%s M=%d G=%d E=%d handed" % (dtype, M, G, E))
            close(out_m, _ref(g, y, w, d, G), *tol, what="%s M=%d G=%d E=%d masked" % (dtype, M, G, E))


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_kernel_single_gaussian_wide_rows_accumulate_guards_empty_and_repeat(dtype):
    from matdeeplearn_amd import ops
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    d_ = dev()
    # G = 1
    g, y, w, d = _operands(65, 64, 1, dtype, seed=3)
    close(ops.linear_dist_grad(g.to(d_), w.to(d_), d.to(d_), act_y=y.to(d_), resolution=1), _ref(g, y, w, d, 1), *tol, what="G=1")
    # ld_g > M: column slices of wider tensors
    E, M, G = 333, 100, 50
    g, y, w, d = _operands(E, M, G, dtype, seed=4, wide=9)
    gs, ys = g.to(d_)[:, 3:3 + M], y.to(d_)[:, 5:5 + M]
    assert gs.stride(0) == M + 9 and not gs.is_contiguous()
    base = ops.linear_dist_grad(gs, w.to(d_), d.to(d_), act_y=ys, resolution=G)
    close(base, _ref(g[:, 3:3 + M], y[:, 5:5 + M], w, d, G), *tol, what="column slices")
    assert torch.equal(base, ops.linear_dist_grad(gs.contiguous(), w.to(d_), d.to(d_), act_y=ys.contiguous(), resolution=G))
    # accumulate onto a non-zero buffer, with guard elements behind E; scale is applied
    big = torch.full((E + 70,), 7.0, device=d_)
    big[:E] = torch.arange(E, device=d_, dtype=torch.float32) * 0.25 - 3.0
    start = big.clone()
    r = ops.linear_dist_grad(gs, w.to(d_), d.to(d_), act_y=ys, resolution=G, out=big[:E])
    assert r.data_ptr() == big.data_ptr()
    assert torch.equal(big[:E], start[:E] + base) and torch.equal(big[E:], start[E:])
    half = ops.linear_dist_grad(gs, w.to(d_), d.to(d_), act_y=ys, resolution=G, scale=0.5)
    close(half, 0.5 * base, 1e-6, 1e-6, what="scale")
    # write mode leaves the guards alone too
    big2 = torch.full((E + 70,), 7.0, device=d_)
    check = ops.linear_dist_grad(gs, w.to(d_), d.to(d_), act_y=ys, resolution=G)
    big2[:E] = check
    assert torch.equal(check, base) and float((big2[E:] - 7.0).abs().max()) == 0.0
    # E = 0: a no-op
    empty = ops.linear_dist_grad(torch.zeros(0, M, device=d_, dtype=dtype), w.to(d_), torch.zeros(0, device=d_), resolution=G)
    assert empty.shape == (0,)
    # bitwise repeatable
    with ops.deterministic():
        a = ops.linear_dist_grad(gs, w.to(d_), d.to(d_), act_y=ys, resolution=G)
        b = ops.linear_dist_grad(gs, w.to(d_), d.to(d_), act_y=ys, resolution=G)
    assert torch.equal(a, b) and torch.equal(a, base)
    with pytest.raises(ops.MdlError):
        ops.linear_dist_grad(torch.zeros(4, 300, device=d_, dtype=dtype), torch.zeros(300, G, device=d_), torch.zeros(4, device=d_), resolution=G)


# ---------------------------------------------------------------------------------------------
# 2. the autograd node
# ---------------------------------------------------------------------------------------------
def _layer_case(E, M, G, dtype, seed):
    gen = torch.Generator().manual_seed(seed)
    w = torch.randn(M, G, generator=gen) * (2.0 / G ** 0.5)
    b = torch.randn(M, generator=gen) * 0.1
    d = torch.rand(E, generator=gen)
    gout = torch.randn(E, M, generator=gen).to(dtype).float()
    return w, b, d, gout


def _oracle_layer_dd(w, b, d, gout, G, rb=lambda t: t):
    dg = d.double().requires_grad_(True)
    y = torch.relu(rb(oops.rbf_expand(dg, 0.0, 1.0, G)) @ rb(w.double()).t() + b.double())
    (g,) = torch.autograd.grad((y * gout.double()).sum(), dg)
    return g


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("M", [64, 100])
def test_node_forward_and_weight_gradients_are_the_layers_own(dtype, M):
    from matdeeplearn_amd import ops
    E, G = 1000, 50
    w, b, d, gout = _layer_case(E, M, G, dtype, seed=M)
    d_ = dev()
    offs = ops.rbf_offsets(0.0, 1.0, G, d_)
    dist_t = d.to(d_).requires_grad_(True)
    ea = ops.rbf_expand(dist_t.detach(), 0.0, 1.0, G, 0.2, out_dtype=dtype, offsets=offs)
    lin = torch.nn.Linear(G, M)
    with torch.no_grad():
        lin.weight.copy_(w); lin.bias.copy_(b)
    lin.to(d_)
    gd = gout.to(d_)

    def old():
        if dtype == torch.float32:
            return torch.relu(torch.nn.functional.linear(ea, lin.weight, lin.bias))
        return ops.linear_act(ea, lin.weight, lin.bias, "relu")

    with ops.deterministic():
        lin.zero_grad(set_to_none=True)
        y0 = old()
        (y0.float() * gd).sum().backward()
        dw0, db0 = lin.weight.grad.clone(), lin.bias.grad.clone()
        lin.zero_grad(set_to_none=True)
        before = ops.LIN_DD_LAUNCHES["distance"]
        y1 = ops.rbf_linear_act(ea, lin.weight, lin.bias, "relu", (dist_t, offs, COEFF))
        (y1.float() * gd).sum().backward()
    assert ops.LIN_DD_LAUNCHES["distance"] == before + 1
    assert y1.dtype == dtype and torch.equal(y0, y1)
    assert torch.equal(lin.weight.grad, dw0) and torch.equal(lin.bias.grad, db0)
    # reference: the fp64 formula on the operands the device multiplied (W in the storage dtype) with the ReLU mask of the device's
    # own output — a unit whose pre-activation rounds across zero (the bias is cast to bf16 too) is a kink of the layer, not an
    # error of the gradient; the fp64 autograd of the unrounded layer is printed next to it
    ref = _ref(gout, y0.float().cpu(), w.to(dtype), d, G)
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    close(dist_t.grad, ref, *tol, what="dd_norm")
    o = _oracle_layer_dd(w, b, d, gout, G)
    print("   against fp64 autograd of the unrounded layer: %.2e of scale" % (float((dist_t.grad.double().cpu() - o).abs().max()) / float(o.abs().max())))
    if dtype == torch.float32:
        close(dist_t.grad, o, *tol, what="dd_norm vs autograd")
    # no gradient asked of the distance: the layer's own path, no launch
    before = ops.LIN_DD_LAUNCHES["distance"]
    y2 = ops.rbf_linear_act(ea, lin.weight, lin.bias, "relu", (dist_t.detach(), offs, COEFF))
    (y2.float() * gd).sum().backward()
    assert torch.equal(y2, y0) and ops.LIN_DD_LAUNCHES["distance"] == before


def test_node_inside_a_fused_bf16_chain_takes_the_handed_down_gradient():
    """nn._seq over Sequential(Linear, ReLU, Linear, ReLU) (MEGNet's edge embedding) on bf16 rows: the first layer's gradient
    arrives w.r.t. its pre-activation; outputs and parameter gradients are those of the chain without dist"""
    from matdeeplearn_amd import nn as mnn, ops
    E, M, G = 1000, 64, 50
    w, b, d, gout = _layer_case(E, M, G, torch.bfloat16, seed=9)
    d_ = dev()
    torch.manual_seed(2)
    seq = torch.nn.Sequential(torch.nn.Linear(G, M), torch.nn.ReLU(), torch.nn.Linear(M, M), torch.nn.ReLU())
    with torch.no_grad():
        seq[0].weight.copy_(w); seq[0].bias.copy_(b)
    ref = copy.deepcopy(seq).double()
    seq.to(d_)
    offs = ops.rbf_offsets(0.0, 1.0, G, d_)
    dist_t = d.to(d_).requires_grad_(True)
    ea = ops.rbf_expand(dist_t.detach(), 0.0, 1.0, G, 0.2, out_dtype=torch.bfloat16, offsets=offs)
    gd = gout.to(d_)
    with ops.deterministic():
        y0 = mnn._seq(seq, ea)
        (y0.float() * gd).sum().backward()
        g0 = [q.grad.clone() for q in seq.parameters()]
        seq.zero_grad(set_to_none=True)
        before = ops.LIN_DD_LAUNCHES["distance"]
        y1 = mnn._seq(seq, ea, dist=(dist_t, offs, COEFF))
        (y1.float() * gd).sum().backward()
    assert ops.LIN_DD_LAUNCHES["distance"] == before + 1 and torch.equal(y0, y1)
    for a, q in zip(g0, seq.parameters()):
        assert torch.equal(a, q.grad)
    # reference: the fp64 formula with the gradient w.r.t. the first layer's pre-activation formed in fp64 from the device's own
    # activations (their ReLU masks; see test_node_forward_and_weight_gradients_are_the_layers_own) and the bf16 weights
    y1 = ops.linear_act(ea, seq[0].weight, seq[0].bias, "relu").float().cpu().double()
    w1, w2 = (seq[k].weight.detach().bfloat16().double().cpu() for k in (0, 2))
    gp = ((gout.double() * (y0.float().cpu() > 0)) @ w2) * (y1 > 0)
    close(dist_t.grad, formula(gp, w1, d.double(), oops.rbf_offsets(0.0, 1.0, G).double(), COEFF), *BF16_TOL, what="dd_norm through the chain")
    dg = d.double().requires_grad_(True)
    (o,) = torch.autograd.grad((ref(oops.rbf_expand(dg, 0.0, 1.0, G)) * gout.double()).sum(), dg)
    print("   against fp64 autograd of the unrounded chain: %.2e of scale" % (float((dist_t.grad.double().cpu() - o).abs().max()) / float(o.abs().max())))


@pytest.mark.parametrize("fused", [True, False])
def test_unsupported_width_and_fused_false_take_the_general_composition(fused):
    from matdeeplearn_amd import _lib, ops
    E, M, G = 500, 300 if fused else 64, 50
    assert bool(_lib.lib().mdl_linear_rbf_dist_grad_supported(M, G, _lib.MDL_F32)) == (not fused)
    w, b, d, gout = _layer_case(E, M, G, torch.float32, seed=M)
    d_ = dev()
    offs = ops.rbf_offsets(0.0, 1.0, G, d_)
    dist_t = d.to(d_).requires_grad_(True)
    ea = ops.rbf_expand(dist_t.detach(), 0.0, 1.0, G, 0.2, offsets=offs)
    wd, bd = w.to(d_).requires_grad_(True), b.to(d_).requires_grad_(True)
    before = ops.LIN_DD_LAUNCHES["distance"]
    y = ops.rbf_linear_act(ea, wd, bd, "relu", (dist_t, offs, COEFF), fused=fused)
    (y * gout.to(d_)).sum().backward()
    assert ops.LIN_DD_LAUNCHES["distance"] == before
    assert torch.equal(y, torch.relu(torch.nn.functional.linear(ea, wd, bd)))
    close(dist_t.grad, _oracle_layer_dd(w, b, d, gout, G), *F32_TOL, what="general composition")


# ---------------------------------------------------------------------------------------------
# 3. end to end
# ---------------------------------------------------------------------------------------------
CASES = {
    "megnet64": ("MEGNet", dict(dim1=64, dim2=64, dim3=64, gc_count=3, post_fc_count=1)),
    "megnet100": ("MEGNet", dict(dim1=100, dim2=100, dim3=100, gc_count=3, gc_fc_count=1, post_fc_count=1)),   # the reference's demo
    "mpnn64": ("MPNN", dict(dim1=64, dim2=64, dim3=64, gc_count=3, post_fc_count=1)),
    "mpnn32x100": ("MPNN", dict(dim1=32, dim2=64, dim3=100, gc_count=3, post_fc_count=1)),
}


def _oracle_data(p, x, s, tg, sh, batch, pos, dtype=torch.float64, rb=lambda t: t):
    d = edge_dist(pos, sh, s, tg).to(dtype)
    dn = (d - DIST_RANGE[0]) / (DIST_RANGE[1] - DIST_RANGE[0])
    B = len(p["node_ptr"]) - 1
    return types.SimpleNamespace(x=rb(x.to(dtype)), edge_index=torch.stack([s, tg]), edge_weight=d, edge_attr=rb(oops.rbf_expand(dn)),
                                 batch=batch, u=torch.zeros(B, 3, dtype=dtype), num_graphs=B)


def _oracle_forces(m, p, ref_in, **kw):
    pos = torch.from_numpy(p["pos"]).requires_grad_(True)
    pred = m(_oracle_data(p, *ref_in, pos, **kw))
    (g,) = torch.autograd.grad(pred.sum(), pos)
    return pred.detach().double(), -g


@functools.lru_cache(maxsize=None)
def _setup(case, mixed):
    """structures, host inputs, the seeded oracle after two optimizer steps (fp32 and fp64 copies) and its fp64 forces: computed
    once per case and shared, never modified"""
    name, kw = CASES[case]
    structs = tgf._mixed_structures() if mixed else tgf._bulk_structures()
    p = tgf._pack(structs)
    ref_in = tgf._reference_inputs(p)
    torch.manual_seed(0)
    ref = getattr(omodels, name)(DS(), **kw)
    data = _oracle_data(p, *ref_in, torch.from_numpy(p["pos"]), dtype=torch.float32)
    y = torch.randn(data.num_graphs, generator=torch.Generator().manual_seed(7))
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    ref.train()
    for _ in range(2):
        opt.zero_grad()
        torch.nn.functional.l1_loss(ref(data), y).backward()
        opt.step()
    ref.eval()
    m64 = copy.deepcopy(ref).double().eval()
    pred64, f64 = _oracle_forces(m64, p, ref_in)
    return structs, p, ref_in, ref, m64, pred64, f64


def _product(case, ref, compute_dtype="fp32"):
    from matdeeplearn_amd import models
    name, kw = CASES[case]
    model = getattr(models, name)(DS(), compute_dtype=compute_dtype, **kw)
    model.load_state_dict(ref.state_dict())
    return model.to(dev()).eval()


@pytest.mark.parametrize("case,mixed", [("megnet64", False), ("megnet64", True), ("megnet100", False),
                                        ("mpnn64", False), ("mpnn64", True), ("mpnn32x100", False)])
def test_energy_and_forces_match_the_fp64_oracle(case, mixed):
    """bound 1e-4 of max|F| (the CGCNN / SchNet force bound).  The fp32 CPU oracle's own distance from the fp64 oracle is printed
    per case: the ReLU models are piecewise smooth, and a seed whose own fp32 sensitivity exceeded 2.5e-5 would be replaced, not
    given a wider bound."""
    from matdeeplearn_amd import forces, ops
    structs, p, ref_in, ref, m64, pred64, f64 = _setup(case, mixed)
    scale = float(f64.abs().max())
    _, f32o = _oracle_forces(ref, p, ref_in, dtype=torch.float32)
    own = float((f32o.double() - f64).abs().max()) / scale
    print("%s mixed=%s: N = %d, fp32 CPU oracle vs fp64 oracle %.2e of max|F|" % (case, mixed, p["pos"].shape[0], own))
    assert own <= 2.5e-5, "pick another seed: this one sits on a ReLU kink in fp32"
    model = _product(case, ref)
    n_layers = 1 if CASES[case][0] == "MEGNet" else CASES[case][1]["gc_count"]
    before = ops.LIN_DD_LAUNCHES["distance"]
    pred, f, node_ptr = forces.energy_and_forces(model, structs, DIST_RANGE)
    assert ops.LIN_DD_LAUNCHES["distance"] == before + n_layers
    assert f.dtype == torch.float32 and f.shape == (p["pos"].shape[0], 3) and torch.equal(node_ptr.cpu(), torch.from_numpy(p["node_ptr"]))
    _check(f, pred, f64, pred64, "fused", tol=1e-4)
    before = ops.LIN_DD_LAUNCHES["distance"]
    pred_u, f_u, _ = forces.energy_and_forces(model, p, DIST_RANGE, fused=False)
    assert ops.LIN_DD_LAUNCHES["distance"] == before                      # no dist on the batch: no new launch
    _check(f_u, pred_u, f64, pred64, "general", tol=1e-4)
    assert torch.equal(pred_u, pred)
    fn = f.double().cpu()
    for b in range(len(structs)):
        fb = fn[p["node_ptr"][b]:p["node_ptr"][b + 1]]
        assert float(fb.sum(0).norm()) <= 1e-5 * float(fb.norm(dim=1).sum()) + 1e-30, b
    if not mixed:
        moved = [dict(s, positions=s["positions"] + s["cell"][k % 3]) for k, s in enumerate(structs)]
        pred_m, f_m, _ = forces.energy_and_forces(model, moved, DIST_RANGE)
        _check(f_m, pred_m, f64, pred64, "shifted by a lattice vector", tol=1e-4)
    with ops.deterministic():
        a = forces.energy_and_forces(model, p, DIST_RANGE)[1]
        b = forces.energy_and_forces(model, p, DIST_RANGE)[1]
    assert torch.equal(a, b)
    assert all(q.grad is None for q in model.parameters())
    # only the expansion route exists: without it the forces are zero, the prediction is the same, and nothing is launched
    before = ops.LIN_DD_LAUNCHES["distance"]
    pred_c, f_c, _ = forces.energy_and_forces(model, p, DIST_RANGE, routes=("cutoff",))
    assert ops.LIN_DD_LAUNCHES["distance"] == before and float(f_c.abs().max()) == 0.0 and torch.equal(pred_c, pred)


@pytest.mark.parametrize("case", ["megnet64", "mpnn64"])
def test_bf16_and_split_mode_forces(case):
    """protocol of test_gpu_schnet_forces.test_schnet_bf16_and_split_mode_forces: the bf16 force error against the fp64 oracle is
    reported and asserted only to be within 4x the oracle's own sensitivity to bf16 storage (fp32 oracle with bf16-rounded
    weights, node and edge features against the fp64 oracle).  A "bf16x3" model keeps fp32 tensors, takes the exact fp32 kernel
    and is held to the fp32 bound."""
    from matdeeplearn_amd import forces, ops
    structs, p, ref_in, ref, m64, pred64, f64 = _setup(case, False)
    scale = float(f64.abs().max())
    mr = copy.deepcopy(ref).eval()
    with torch.no_grad():
        for q in mr.parameters():
            if q.dim() == 2:
                q.copy_(q.bfloat16().float())
    rb = lambda t: t + (t.detach().bfloat16().to(t.dtype) - t.detach())
    _, fr = _oracle_forces(mr, p, ref_in, dtype=torch.float32, rb=rb)
    sens = float((fr.double() - f64).abs().max()) / scale
    n_layers = 1 if CASES[case][0] == "MEGNet" else CASES[case][1]["gc_count"]
    model = _product(case, ref, "bf16")
    before = ops.LIN_DD_LAUNCHES["distance"]
    pred, f, _ = forces.energy_and_forces(model, structs, DIST_RANGE)
    assert ops.LIN_DD_LAUNCHES["distance"] == before + n_layers
    err = float((f.double().cpu() - f64).abs().max()) / scale
    f_u = forces.energy_and_forces(model, structs, DIST_RANGE, fused=False)[1]
    err_u = float((f_u.double().cpu() - f64).abs().max()) / scale
    print("bf16 %s: oracle bf16-storage sensitivity %.3e of max|F|, force error %.3e of max|F| (bound %.3e); general route %.3e"
          % (case, sens, err, 4 * sens, err_u))
    assert err <= 4 * sens
    m3 = _product(case, ref, "bf16x3")
    before = ops.LIN_DD_LAUNCHES["distance"]
    pred3, f3, _ = forces.energy_and_forces(m3, structs, DIST_RANGE)
    assert ops.LIN_DD_LAUNCHES["distance"] == before + n_layers
    _check(f3, pred3, f64, pred64, "bf16x3 (exact fp32 form)", tol=1e-4)
