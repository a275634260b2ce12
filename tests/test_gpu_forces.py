"""GPU checks of the derivative path  positions -> distances -> Gaussian expansion -> CGConv / CGCNN:  the CGConv edge-feature
gradient (general and fused distance epilogue of csrc/cgconv_de.hip), the expansion's backward, the edge geometry and
matdeeplearn_amd.forces.energy_and_forces.

Reference: the project's CPU oracle under autograd (oracle.ops.cgconv / rbf_expand, oracle.models.CGCNN are pure torch), with the
geometry helper this file owns (minimum-image shifts from one no-grad pass, then |p_tgt + shift - p_src| under autograd;
tests/test_forces_host.py checks the same helper and the oracle force formula against central differences).  The upstream
reference has no force path, so no golden from it exists.  Self-contained: this file sorts in front of test_gpu_kernels.py."""
import os
import types

import numpy as np
import pytest
import torch

from oracle import models as omodels
from oracle import ops as oops

pytestmark = pytest.mark.gpu
G_DIR = os.path.join(os.path.dirname(__file__), "golden")
F32_TOL = (2e-5, 2e-5)        # the project's fp32 kernel bound (tests/test_gpu_kernels.py)
BF16_TOL = (3e-2, 3e-2)       # and its bf16 bound


def dev():
    return torch.device("cuda:0")


def close(a, b, rtol, atol_scale, what=""):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    scale = float(b.abs().max()) + 1e-30
    err = float((a - b).abs().max())
    print("%s max abs err %.3e scale %.3e (%.2e of scale; bound %.1e)" % (what, err, scale, err / scale, atol_scale))
    assert torch.allclose(a, b, rtol=rtol, atol=atol_scale * scale), "%s max abs err %.3e (scale %.3e)" % (what, err, scale)


def rand_graph(n, seed, max_in=20, window=40, empty_frac=0.1, sort=False):
    """the random graphs of tests/test_gpu_kernels.py (same draws)"""
    g = torch.Generator().manual_seed(seed)
    src, tgt = [], []
    for i in range(n):
        if torch.rand(1, generator=g).item() < empty_frac:
            continue
        k = int(torch.randint(1, max_in + 1, (1,), generator=g))
        s = torch.randint(max(0, i - window), min(n, i + window), (k,), generator=g).tolist()
        s.append(i)
        src += s
        tgt += [i] * len(s)
    ei = torch.tensor([src, tgt], dtype=torch.int64)
    if not sort:
        ei = ei[:, torch.randperm(ei.shape[1], generator=g)]
    return ei


def _layer_inputs(n, C, G, dtype, sort, seed, empty_frac=0.1, window=40):
    """inputs of one layer, rounded to the storage dtype first, exactly as _cgconv_case of tests/test_gpu_kernels.py draws them"""
    g = torch.Generator().manual_seed(seed)
    ei = rand_graph(n, seed, sort=sort, empty_frac=empty_frac, window=window)
    E = ei.shape[1]
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(n, C).to(dtype).float()
    ea = torch.rand(E, G, generator=g).to(dtype).float()
    k = 1.0 / (2 * C + G) ** 0.5
    wf, ws = (rnd(C, 2 * C + G) * k * 3).to(dtype).float(), (rnd(C, 2 * C + G) * k * 3).to(dtype).float()
    bf, bs = rnd(C) * 0.1, rnd(C) * 0.1
    gout = rnd(n, C).to(dtype).float()
    return ei, x, ea, wf, bf, ws, bs, gout


# ---------------------------------------------------------------------------------------------
# 1. de vs oracle
# ---------------------------------------------------------------------------------------------
def _de_case(n, C, G, dtype, sort, seed, aggr="mean", empty_frac=0.1, window=40):
    from matdeeplearn_amd import ops
    ei, x, ea, wf, bf, ws, bs, gout = _layer_inputs(n, C, G, dtype, sort, seed, empty_frac, window)
    xo, eo, wfo, wso, bfo, bso = [t.clone().requires_grad_(True) for t in (x, ea, wf, ws, bf, bs)]
    ref = oops.cgconv(xo, ei, eo, wfo, bfo, wso, bso, aggr)
    (ref * gout).sum().backward()

    d = dev()
    xd = x.to(d).to(dtype).requires_grad_(True)
    ed = ea.to(d).to(dtype).requires_grad_(True)
    wfd, wsd, bfd, bsd = [t.to(d).clone().requires_grad_(True) for t in (wf, ws, bf, bs)]
    csr = ops.build_csr(ei.to(d), n, assume_sorted=sort)
    out = ops.cgconv(xd, ei.to(d), ed, wfd, bfd, wsd, bsd, aggr, csr=csr)
    (out.float() * gout.to(d)).sum().backward()
    tol = F32_TOL if dtype == torch.float32 else BF16_TOL
    assert ed.grad is not None and ed.grad.dtype == dtype and ed.grad.shape == ed.shape
    close(ed.grad, eo.grad, *tol, what="de")
    close(out, ref, *tol, what="out")                          # in the same call the other five gradients still meet the bound
    close(xd.grad, xo.grad, *tol, what="dx")
    close(wfd.grad, wfo.grad, *tol, what="dW_f")
    close(wsd.grad, wso.grad, *tol, what="dW_s")
    close(bfd.grad, bfo.grad, *tol, what="db_f")
    close(bsd.grad, bso.grad, *tol, what="db_s")


SPARSE_N, SPARSE_EMPTY = 2000, 0.93      # the sparse graph of tests/test_gpu_kernels.py: 93 % of 2000 nodes without edges


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("n,C,G,sort", [(200, 64, 50, True), (200, 64, 50, False), (77, 32, 50, True),
                                         (130, 100, 50, False), (65, 128, 50, True), (900, 100, 50, True), (50, 64, 41, True),
                                         (33, 20, 7, False), (1, 64, 50, True),
                                         # bias from bpack (G % 16 == 0), element loads of x (C % 4 != 0), N > E with most nodes isolated
                                         (200, 64, 64, True), (100, 32, 16, True), (100, 30, 7, True), (SPARSE_N, 64, 50, True)])
def test_cgconv_edge_attr_gradient_matches_oracle(dtype, n, C, G, sort):
    _de_case(n, C, G, dtype, sort, seed=n + C + G, empty_frac=SPARSE_EMPTY if n == SPARSE_N else 0.1)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cgconv_edge_attr_gradient_add_aggr_isolated_nodes_wide_window(dtype):
    _de_case(150, 64, 50, dtype, True, seed=5, aggr="add", empty_frac=0.5)
    _de_case(1500, 64, 50, dtype, True, seed=35, empty_frac=0.0, window=400)


def test_cgconv_edge_attr_gradient_no_edges_and_double_backward():
    from matdeeplearn_amd import ops
    d = dev()
    x = torch.randn(5, 64, device=d, requires_grad=True)
    ea = torch.zeros(0, 50, device=d, requires_grad=True)
    ei = torch.zeros(2, 0, dtype=torch.int64, device=d)
    w = [torch.randn(64, 178, device=d) * 0.1 for _ in range(2)]
    out = ops.cgconv(x, ei, ea, w[0], None, w[1], None, "mean", csr=ops.build_csr(ei, 5, assume_sorted=True))
    out.sum().backward()
    assert ea.grad is not None and ea.grad.shape == (0, 50)
    # a second differentiation raises instead of returning silence
    ei2 = rand_graph(40, 1, sort=True).to(d)
    e2 = torch.rand(ei2.shape[1], 50, device=d, requires_grad=True)
    x2 = torch.randn(40, 64, device=d, requires_grad=True)
    o2 = ops.cgconv(x2, ei2, e2, w[0], None, w[1], None, "mean", csr=ops.build_csr(ei2, 40, assume_sorted=True))
    (g,) = torch.autograd.grad(o2.sum(), e2, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---------------------------------------------------------------------------------------------
# 2. fused distance epilogue vs oracle
# ---------------------------------------------------------------------------------------------
def _oracle_dd(x, ei, d, wf, bf, ws, bs, gout, aggr, G, round_bf16=False):
    """dL/dd_norm through oracle.rbf_expand + oracle.cgconv in the dtype of the arguments; round_bf16: x, e, W rounded to bf16
    (straight-through: the rounding passes the gradient) — the reference's own sensitivity to the storage rounding"""
    rb = (lambda t: t + (t.detach().to(torch.bfloat16).to(t.dtype) - t.detach())) if round_bf16 else (lambda t: t)
    dg = d.clone().requires_grad_(True)
    out = oops.cgconv(rb(x), ei, rb(oops.rbf_expand(dg, 0.0, 1.0, G, 0.2)), rb(wf), bf, rb(ws), bs, aggr)
    (out * gout).sum().backward()
    return dg.grad


def _dist_case(n, C, G, dtype, sort, seed, aggr="mean"):
    from matdeeplearn_amd import ops
    ei, x, _, wf, bf, ws, bs, gout = _layer_inputs(n, C, G, torch.float32, sort, seed)
    gout = gout.to(torch.bfloat16).float()                 # representable in both storage dtypes: grad_out is not what gets rounded
    dn = torch.rand(ei.shape[1], generator=torch.Generator().manual_seed(seed + 1))
    ref64 = _oracle_dd(*[t.double() if t.is_floating_point() else t for t in (x, ei, dn, wf, bf, ws, bs, gout)], aggr, G)
    scale = float(ref64.abs().max())
    if dtype == torch.float32:
        ref32 = _oracle_dd(x, ei, dn, wf, bf, ws, bs, gout, aggr, G)
        ref_err = float((ref32.double() - ref64).abs().max()) / scale
        bound = 2e-5 if ref_err <= 5e-6 else 4 * ref_err
    else:
        ref_err = float((_oracle_dd(x, ei, dn, wf, bf, ws, bs, gout, aggr, G, round_bf16=True).double() - ref64).abs().max()) / scale
        bound = 4 * ref_err
    print("reference-vs-reference error %.3e of scale -> bound %.3e" % (ref_err, bound))
    d = dev()
    csr = ops.build_csr(ei.to(d), n, assume_sorted=sort)
    dd = ops.cgconv_dist_grad(x.to(d).to(dtype), ei.to(d), dn.to(d), wf.to(d), bf.to(d), ws.to(d), bs.to(d), gout.to(d), aggr, csr=csr,
                              resolution=G)
    assert dd.dtype == torch.float32 and dd.shape == dn.shape
    close(dd, ref64, bound, bound, what="dd")
    # the autograd route of the same epilogue (ops.cgconv(dist=...)): the same launch, the same bits
    xd = x.to(d).to(dtype)
    dg = dn.to(d).requires_grad_(True)
    offs = ops.rbf_offsets(0.0, 1.0, G, d)
    ea = ops.rbf_expand(dg.detach(), 0.0, 1.0, G, 0.2, out_dtype=dtype, offsets=offs)
    out = ops.cgconv(xd, ei.to(d), ea, wf.to(d), bf.to(d), ws.to(d), bs.to(d), aggr, csr=csr, dist=(dg, offs, ops.rbf_coeff(0.0, 1.0, 0.2)))
    (out.float() * gout.to(d)).sum().backward()
    assert torch.equal(dg.grad, dd)
    # scale and accumulation into a caller's buffer (CSR-ordered edge lists)
    if sort:
        buf = torch.ones_like(dd)
        ops.cgconv_dist_grad(xd, ei.to(d), dn.to(d), wf.to(d), bf.to(d), ws.to(d), bs.to(d), gout.to(d), aggr, csr=csr, resolution=G,
                             scale=0.5, out=buf)
        close(buf - 1.0, 0.5 * dd, 1e-6, 1e-6, what="scaled dd")


@pytest.mark.parametrize("n,C,G,sort,aggr", [(200, 64, 50, True, "mean"), (200, 64, 50, False, "mean"), (130, 100, 50, False, "add"),
                                              (33, 20, 7, False, "mean"), (900, 100, 50, True, "mean"), (50, 64, 41, True, "add"),
                                              (200, 64, 64, True, "mean")])        # G % 16 == 0: the bias from bpack under the fused epilogue
def test_cgconv_distance_epilogue_matches_oracle_fp32(n, C, G, sort, aggr):
    """dL/dd_norm of one layer through rbf_expand + cgconv: bound close(2e-5, 2e-5) — kept where the fp32 CPU oracle agrees with the
    fp64 CPU oracle to 5e-6 of the scale, else 4x that reference-vs-reference error.  Measured on the CPU for these cases: the fp32
    oracle differs from the fp64 oracle by 2.3e-7 .. 9.1e-7 of the scale, so the bound is 2e-5 in all of them."""
    _dist_case(n, C, G, torch.float32, sort, seed=n + C + G, aggr=aggr)


@pytest.mark.parametrize("n,C,G,sort,aggr", [(200, 64, 50, True, "mean"), (130, 100, 50, False, "add"), (33, 20, 7, False, "mean")])
def test_cgconv_distance_epilogue_bf16_within_the_references_own_sensitivity(n, C, G, sort, aggr):
    """bf16 storage has no pre-set bound.  The reference's own sensitivity to the storage rounding — fp32 CPU oracle on bf16-rounded
    x, e, W against the fp64 oracle on the unrounded values — is measured in the test (on the CPU for these three cases: 3.4e-3,
    2.4e-3 and 4.1e-3 of the scale); the kernel, which also rounds dpre to bf16 for its second product, is allowed 4x that
    (1.4e-2, 9.7e-3, 1.6e-2).  grad_out is drawn bf16-representable, so the rounded quantities are exactly x, e and W."""
    _dist_case(n, C, G, torch.bfloat16, sort, seed=n + C + G, aggr=aggr)


# ---------------------------------------------------------------------------------------------
# 3. rbf_expand backward
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rbf_expand_backward_matches_oracle(dtype):
    from matdeeplearn_amd import ops
    dn = torch.from_numpy(np.load(os.path.join(G_DIR, "rbf.npz"))["d"]).float()
    w = torch.randn(dn.numel(), 50, generator=torch.Generator().manual_seed(0)).to(dtype).float()
    do = dn.double().requires_grad_(True)
    (oops.rbf_expand(do) * w.double()).sum().backward()
    dg = dn.to(dev()).requires_grad_(True)
    out = ops.rbf_expand(dg, out_dtype=dtype)
    assert out.dtype == dtype and torch.equal(out, ops.rbf_expand(dg.detach(), out_dtype=dtype))     # the forward launch is today's
    out.backward(w.to(dev()).to(dtype))
    close(dg.grad, do.grad, *F32_TOL, what="rbf dd")
    (g,) = torch.autograd.grad(ops.rbf_expand(dg).sum(), dg, create_graph=True)
    with pytest.raises(RuntimeError):
        g.sum().backward()


# ---------------------------------------------------------------------------------------------
# geometry helper (the same code as tests/test_forces_host.py, which checks it against finite differences)
# ---------------------------------------------------------------------------------------------
def edge_shifts(pos, node_ptr, cell, pbc, src, tgt):
    pos, cell = np.asarray(pos, np.float64), np.asarray(cell, np.float64)
    g = np.searchsorted(np.asarray(node_ptr), np.asarray(src), side="right") - 1
    n = np.stack(np.meshgrid(*[np.arange(-2, 3)] * 3, indexing="ij"), -1).reshape(-1, 3)
    per = ((np.asarray(pbc)[g][:, None] >> np.arange(3)[None, :]) & 1).astype(bool)
    ok = (~(n[None, :, :] != 0) | per[:, None, :]).all(-1)
    out = np.zeros((len(g), 3))
    for a in range(0, len(g), 4096):                      # chunks: [E, 125, 3] doubles
        b = slice(a, a + 4096)
        sh = np.einsum("ka,eab->ekb", n.astype(np.float64), cell[g[b]])
        d0 = pos[np.asarray(tgt)[b]] - pos[np.asarray(src)[b]]
        r2 = ((d0[:, None, :] + sh) ** 2).sum(-1)
        r2[~ok[b]] = np.inf
        out[b] = sh[np.arange(sh.shape[0]), r2.argmin(1)]
    return out


def edge_dist(pos, shift, src, tgt):
    v = pos.index_select(0, tgt) + shift - pos.index_select(0, src)
    r2 = (v * v).sum(1)
    ok = r2 > 0
    return torch.zeros_like(r2).masked_scatter(ok, torch.sqrt(r2[ok]))


def _pack(structs):
    from matdeeplearn_amd.process import graph as pg
    return pg.pack_structures(structs)


def _graphs(p, radius=8.0, k=12):
    """build_graphs on the device; batch-global edge ids on the host"""
    from matdeeplearn_amd import ops
    d = dev()
    t = {key: torch.from_numpy(p[key]).to(d) for key in ("pos", "node_ptr", "cell", "pbc")}
    edge_ptr, src, tgt, dist, out_deg = ops.build_graphs(t["pos"], t["node_ptr"], t["cell"], t["pbc"], radius, k)
    shift = torch.repeat_interleave(t["node_ptr"][:-1], edge_ptr[1:] - edge_ptr[:-1]).to(torch.int32)
    return t, edge_ptr, src, tgt, dist, out_deg, src + shift, tgt + shift


def _mixed_structures(seed=0):
    rng = np.random.default_rng(seed)
    out = []
    for s in range(72):
        kind = s % 4
        n = int(rng.integers(2, 30))
        if kind == 0:      # orthorhombic
            cell, pbc = np.diag(rng.uniform(5.0, 9.0, 3)), [True, True, True]
        elif kind == 1:    # triclinic, mild skew
            cell = np.diag(rng.uniform(6.0, 9.0, 3)) + np.tril(rng.uniform(-1.5, 1.5, (3, 3)), -1)
            pbc = [True, True, True]
        elif kind == 2:    # slab
            cell, pbc = np.diag([rng.uniform(5.0, 8.0), rng.uniform(5.0, 8.0), 20.0]), [True, True, False]
        else:              # molecule
            cell, pbc = np.zeros((3, 3)), [False, False, False]
        box = cell if kind != 3 else np.eye(3) * 6.0
        pos = rng.uniform(0, 1, (n, 3)) @ box
        if kind == 2:
            pos[:, 2] = rng.uniform(0, 6.0, n)
        out.append({"positions": pos, "numbers": rng.integers(1, 90, n), "cell": cell, "pbc": pbc})
    out.append({"positions": np.array([[1.0, 2.0, 3.0]]), "numbers": [8], "cell": np.eye(3) * 5.0, "pbc": [True] * 3})     # one atom
    pair = rng.uniform(0, 5.0, (4, 3))
    pair[1] = pair[0]                                                                                                     # coincident pair
    out.append({"positions": pair, "numbers": [1, 1, 6, 8], "cell": np.eye(3) * 6.0, "pbc": [True] * 3})
    return out


# ---------------------------------------------------------------------------------------------
# 4. geometry
# ---------------------------------------------------------------------------------------------
def test_edge_vectors_reproduce_the_builder_and_differentiate():
    from matdeeplearn_amd import ops
    p = _pack(_mixed_structures())
    t, edge_ptr, src_l, tgt_l, dist_b, _, src, tgt = _graphs(p)
    assert len(p["node_ptr"]) - 1 >= 64
    pos = t["pos"].clone().requires_grad_(True)
    dist, u = ops.edge_vectors(pos, t["node_ptr"], t["cell"], t["pbc"], src_l, tgt_l, edge_ptr=edge_ptr, return_unit=True)
    assert torch.equal(dist, dist_b)                                   # bitwise the builder's distances
    dist_g = ops.edge_vectors(t["pos"], t["node_ptr"], t["cell"], t["pbc"], src, tgt)          # batch-global ids: the same
    assert torch.equal(dist_g, dist_b)
    loops = (src == tgt) | (dist_b == 0)
    assert int((src == tgt).sum()) == pos.shape[0]
    assert float(u[loops].abs().max()) == 0.0
    assert float((u[~loops].double().norm(dim=1) - 1.0).abs().max()) <= 1e-6
    # backward against the fp64 helper
    w = torch.randn(dist.numel(), generator=torch.Generator().manual_seed(1))
    dist.backward(w.to(dev()))
    sh = torch.from_numpy(edge_shifts(p["pos"], p["node_ptr"], p["cell"], p["pbc"], src.cpu().numpy(), tgt.cpu().numpy()))
    p64 = torch.from_numpy(p["pos"]).requires_grad_(True)
    d64 = edge_dist(p64, sh, src.cpu().long(), tgt.cpu().long())
    close(dist, d64, 1e-6, 1e-7, what="dist vs helper")
    (d64 * w.double()).sum().backward()
    assert pos.grad.dtype == torch.float64
    close(pos.grad, p64.grad, *F32_TOL, what="dpos")
    # an unsorted edge list goes through the sorts of the backward and gives the same gradient
    perm = torch.randperm(src.numel(), generator=torch.Generator().manual_seed(2)).to(dev())
    pos2 = t["pos"].clone().requires_grad_(True)
    d2 = ops.edge_vectors(pos2, t["node_ptr"], t["cell"], t["pbc"], src[perm].contiguous(), tgt[perm].contiguous())
    assert torch.equal(d2, dist_b[perm])
    d2.backward(w.to(dev())[perm])
    close(pos2.grad, p64.grad, *F32_TOL, what="dpos (unsorted)")
    with ops.deterministic():
        pos3 = t["pos"].clone().requires_grad_(True)
        ops.edge_vectors(pos3, t["node_ptr"], t["cell"], t["pbc"], src, tgt).backward(w.to(dev()))
        assert torch.equal(pos3.grad, pos.grad)


# ---------------------------------------------------------------------------------------------
# 5. / 6. end to end
# ---------------------------------------------------------------------------------------------
class DS:
    num_features, num_edge_features = 114, 50

    def __getitem__(self, i):
        return types.SimpleNamespace(y=torch.tensor(0.0), u=torch.zeros(1, 3))


def _bulk_structures(n_structs=32, seed=0, lo=4, hi=40):
    """drawn the way process.dataset.synthetic_bulk draws them: cubic periodic cell at density 0.05, uniform positions, Z in 1..89"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n_structs):
        n = int(rng.integers(lo, hi + 1))
        L = (n / 0.05) ** (1.0 / 3.0)
        out.append({"positions": rng.uniform(0.0, 1.0, (n, 3)) * L, "numbers": rng.integers(1, 90, n), "cell": np.eye(3) * L,
                    "pbc": [True, True, True]})
    return out


DIST_RANGE = (0.0, 8.0)


def _reference_inputs(p):
    """topology from the device builder, everything else on the host: x, batch-global edge_index, image shifts"""
    from matdeeplearn_amd import forces
    t, _, _, _, _, out_deg, src, tgt = _graphs(p)
    x = forces._node_features(p["numbers"], out_deg, 12, None, dev()).cpu()
    s, tg = src.cpu().long(), tgt.cpu().long()
    sh = torch.from_numpy(edge_shifts(p["pos"], p["node_ptr"], p["cell"], p["pbc"], s.numpy(), tg.numpy()))
    batch = torch.from_numpy(np.repeat(np.arange(len(p["node_ptr"]) - 1), np.diff(p["node_ptr"])))
    return x, s, tg, sh, batch


def _oracle_forces(m64, p, x, s, tg, sh, batch):
    pos = torch.from_numpy(p["pos"]).requires_grad_(True)
    d = edge_dist(pos, sh, s, tg)
    data = types.SimpleNamespace(x=x.double(), edge_index=torch.stack([s, tg]),
                                 edge_attr=oops.rbf_expand((d - DIST_RANGE[0]) / (DIST_RANGE[1] - DIST_RANGE[0])), batch=batch,
                                 num_graphs=len(p["node_ptr"]) - 1)
    pred = m64(data)
    (g,) = torch.autograd.grad(pred.sum(), pos)
    return pred.detach(), -g


def _trained_models(dim, p, x, s, tg, sh, batch):
    """seeded CGCNN, two optimizer steps on the CPU oracle (so the running statistics are not the initial ones), eval mode"""
    from matdeeplearn_amd import models
    torch.manual_seed(0)
    kw = dict(dim1=dim, dim2=dim, gc_count=4, post_fc_count=1)
    ref = omodels.CGCNN(DS(), **kw)
    with torch.no_grad():
        d = edge_dist(torch.from_numpy(p["pos"]), sh, s, tg).float()
    data = types.SimpleNamespace(x=x, edge_index=torch.stack([s, tg]), edge_attr=oops.rbf_expand(d / 8.0), batch=batch,
                                 num_graphs=len(p["node_ptr"]) - 1)
    y = torch.randn(data.num_graphs, generator=torch.Generator().manual_seed(7))
    opt = torch.optim.Adam(ref.parameters(), lr=1e-3)
    ref.train()
    for _ in range(2):
        opt.zero_grad()
        torch.nn.functional.l1_loss(ref(data), y).backward()
        opt.step()
    ref.eval()
    model = models.CGCNN(DS(), **kw)
    model.load_state_dict(ref.state_dict())
    model.to(dev()).eval()
    import copy
    return model, copy.deepcopy(ref).double().eval()


def _check_forces(f, pred, f64, pred64, what):
    scale = float(f64.abs().max())
    ferr = float((f.double().cpu() - f64).abs().max())
    print("%s: max|F| %.3e, max force error %.3e (%.2e of max|F|; bound 1e-4)" % (what, scale, ferr, ferr / scale))
    assert torch.allclose(pred.double().cpu(), pred64, rtol=1e-4, atol=1e-4 * float(pred64.abs().max())), what
    assert torch.allclose(f.double().cpu(), f64, rtol=1e-4, atol=1e-4 * scale), "%s: force error %.3e (max|F| %.3e)" % (what, ferr, scale)


@pytest.mark.parametrize("dim", [64, 100])
def test_energy_and_forces_match_the_fp64_oracle(dim):
    from matdeeplearn_amd import forces, ops
    structs = _bulk_structures()
    p = _pack(structs)
    ref_in = _reference_inputs(p)
    model, m64 = _trained_models(dim, p, *ref_in)
    pred64, f64 = _oracle_forces(m64, p, *ref_in)
    pred, f, node_ptr = forces.energy_and_forces(model, structs, DIST_RANGE)
    assert f.dtype == torch.float32 and f.shape == (p["pos"].shape[0], 3) and torch.equal(node_ptr.cpu(), torch.from_numpy(p["node_ptr"]))
    _check_forces(f, pred, f64, pred64, "fused")
    # the unfused composition edge_vectors -> rbf_expand -> model (an [E, G] gradient per layer + the expansion's backward)
    pred_u, f_u, _ = forces.energy_and_forces(model, p, DIST_RANGE, fused=False)
    _check_forces(f_u, pred_u, f64, pred64, "unfused")
    assert torch.equal(pred_u, pred)
    # 6. invariants: no net force on a graph
    fn = f.double().cpu()
    for b in range(len(structs)):
        fb = fn[p["node_ptr"][b]:p["node_ptr"][b + 1]]
        assert float(fb.sum(0).norm()) <= 1e-5 * float(fb.norm(dim=1).sum()) + 1e-30, b
    # shifting every position of a periodic structure by a lattice vector leaves the forces where they were
    moved = [dict(s, positions=s["positions"] + s["cell"][k % 3]) for k, s in enumerate(structs)]
    pred_m, f_m, _ = forces.energy_and_forces(model, moved, DIST_RANGE)
    _check_forces(f_m, pred_m, f64, pred64, "shifted by a lattice vector")
    # bitwise repeatable in deterministic mode
    with ops.deterministic():
        a = forces.energy_and_forces(model, p, DIST_RANGE)[1]
        b = forces.energy_and_forces(model, p, DIST_RANGE)[1]
    assert torch.equal(a, b)
    # nothing was left behind on the parameters
    assert all(q.grad is None for q in model.parameters())


def test_energy_and_forces_output_index_and_mode():
    from matdeeplearn_amd import forces, models, ops

    class DS2(DS):
        def __getitem__(self, i):
            return types.SimpleNamespace(y=torch.zeros(1, 2), u=torch.zeros(1, 3))

    torch.manual_seed(1)
    model = models.CGCNN(DS2(), dim1=64, dim2=64, gc_count=2, post_fc_count=1).to(dev()).eval()
    structs = _bulk_structures(6, seed=3)
    pred, f_sum, _ = forces.energy_and_forces(model, structs, DIST_RANGE)
    assert pred.shape == (6, 2)
    f0 = forces.energy_and_forces(model, structs, DIST_RANGE, output_index=0)[1]
    f1 = forces.energy_and_forces(model, structs, DIST_RANGE, output_index=1)[1]
    close(f0 + f1, f_sum, 1e-4, 1e-5, what="sum over outputs")
    with pytest.raises(ops.MdlError, match="CGCNN"):
        forces.energy_and_forces(models.SchNet(DS(), dim1=64, dim2=64, dim3=64, gc_count=1), structs, DIST_RANGE)


# ---------------------------------------------------------------------------------------------
# 7. nothing else moved
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cgconv_without_edge_gradient_is_what_it_was(dtype):
    from matdeeplearn_amd import ops
    ei, x, ea, wf, bf, ws, bs, gout = _layer_inputs(300, 64, 50, dtype, True, 11)
    d = dev()
    csr = ops.build_csr(ei.to(d), 300, assume_sorted=True)

    def run(edge_grad):
        xd = x.to(d).to(dtype).requires_grad_(True)
        ed = ea.to(d).to(dtype).requires_grad_(edge_grad)
        ps = [t.to(d).clone().requires_grad_(True) for t in (wf, bf, ws, bs)]
        out = ops.cgconv(xd, ei.to(d), ed, ps[0], ps[1], ps[2], ps[3], "mean", csr=csr)
        (out.float() * gout.to(d)).sum().backward()
        return [out.detach(), xd.grad] + [q.grad for q in ps], ed.grad

    with ops.deterministic():
        a, ga = run(False)
        b, gb = run(False)
        c, gc = run(True)
    assert ga is None and gb is None and gc is not None
    for u, v, w in zip(a, b, c):
        assert torch.equal(u, v) and torch.equal(u, w)         # asking for the edge gradient does not move the other results either
