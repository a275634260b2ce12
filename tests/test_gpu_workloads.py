"""GPU parity on the BASELINE.json workloads, product (HIP) against the oracle (CPU) on the SAME batches:

  cfg2  synthetic bulk-like graphs (1..200 atoms, graphs wider than the backward's 64-node source window included),
        CGCNN dim 64 x 4 conv: kernel level (forward + every gradient, fp32 and bf16, large enough for the backward's
        dynamic group schedule) and model level (prediction / val-MAE at fixed weights, fp32 and bf16)
  cfg3  synthetic MOF-like graphs (20..500 atoms: long segments, sources far outside any window), SchNet_demo
        hyper-parameters of the reference's config.yml:162-183 (dim1 100, dim2 100, dim3 150, 4 interaction blocks)
  cfg4  bulk-like graphs, MEGNet_demo hyper-parameters (config.yml:184-205: dims 100, 4 blocks, gc_fc_count 1)
  cfg5  surface-like slabs, the five-model ensemble driver on the device against the same driver on the oracle

Tolerances (stated once): fp32 predictions 1e-4 of the tensor scale and |dMAE| < 1e-5 against the oracle in fp64 (the fp32
oracle's own rounding error reaches that size: MEGNet_demo's train-mode prediction differs from fp64 by 1e-4 of its scale on 16
CPU threads and 3e-3 on one, the HIP path by 2e-5); fp32 gradients no worse than
50 x the fp32-CPU error against an fp64 truth (floor 2e-4 of the scale; mse loss so that the gradient is smooth); bf16 predictions 5e-2 of the scale,
bf16 kernel outputs / gradients 3e-2 of the scale (inputs pre-rounded to bf16 on both sides).
"""
import copy
import types

import numpy as np
import pytest
import torch

from oracle import models as omodels
from oracle import ops as oops

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _cpu_twin(ds):
    c = copy.copy(ds)
    c._dev = {}
    c.to("cpu")
    return c


def _composition_targets(ds):
    """A target the models can actually fit (mean atomic number of the graph, standardised): with the recipe's N(0,1)
    noise targets every model scores MAE ~ E|y| and an MAE comparison could not tell two models apart."""
    z = np.add.reduceat(ds.z.astype(np.float64), ds.node_ptr[:-1]) / np.diff(ds.node_ptr)
    ds.y = ((z - z.mean()) / z.std()).astype(np.float32).reshape(-1, 1)
    return ds


def _batches(ds, ids, dtype=torch.float32):
    rbf = lambda d: oops.rbf_expand(d, 0.0, 1.0, ds.num_edge_features, 0.2)
    bc = _cpu_twin(ds).collate(ids, rbf=rbf)
    bg = ds.collate(ids, edge_dtype=dtype, x_dtype=dtype)
    return bc, bg


def _close(a, b, rel, what=""):
    a, b = a.detach().float().cpu(), b.detach().float().cpu()
    s = float(b.abs().max()) + 1e-12
    err = float((a - b).abs().max())
    assert err <= rel * s, "%s: max err %.3e vs scale %.3e (allowed %.1e of scale)" % (what, err, s, rel)


def _model_parity(name, kw, ds, ids, grads=True):
    """fp32 product vs the oracle (same state_dict, same batch): train-mode prediction and gradients against the fp64
    oracle (gradients no worse than a multiple of the fp32 oracle's error), eval-mode prediction / MAE against the fp64
    oracle; then the bf16 product against the fp32 oracle's prediction."""
    from matdeeplearn_amd import models
    torch.manual_seed(0)
    ref_model = getattr(omodels, name)(ds, **kw)
    model = getattr(models, name)(ds, **kw)
    assert list(model.state_dict()) == list(ref_model.state_dict())
    model.load_state_dict(ref_model.state_dict())
    model.to(DEV)
    m64 = copy.deepcopy(ref_model).double()
    bc, bg = _batches(ds, ids)
    b64 = types.SimpleNamespace(**{k: (v.double() if torch.is_tensor(v) and v.is_floating_point() else v)
                                   for k, v in vars(bc).items() if not k.startswith("_")})
    b64.edge_index = bc.edge_index
    ref_model.train(); model.train(); m64.train()
    # (mse for the gradient comparison: the l1 gradient is sign(out - y), which flips on rounding noise whenever a
    # prediction happens to sit on its target — a discrete jump no tolerance can absorb)
    ref = ref_model(bc)
    torch.nn.functional.mse_loss(ref, bc.y).backward()
    out = model(bg)
    torch.nn.functional.mse_loss(out, bg.y).backward()
    out64 = m64(b64)
    _close(out, out64, 1e-4, name + " fp32 train prediction")
    if grads:
        torch.nn.functional.mse_loss(out64, b64.y).backward()
        rg, g64 = dict(ref_model.named_parameters()), dict(m64.named_parameters())
        gmax = max(float(v.grad.abs().max()) for v in g64.values() if v.grad is not None)    # floor for near-zero gradients
        for k, p in model.named_parameters():
            if g64[k].grad is None:
                continue
            truth = g64[k].grad
            s = float(truth.abs().max()) + 1e-12
            cpu_err = float((rg[k].grad.double() - truth).abs().max())
            gpu_err = float((p.grad.cpu().double() - truth).abs().max()) if p.grad is not None else s
            # (50 x the fp32-CPU error, with a floor of 2e-4 of the model's largest gradient: the MLPs' ReLUs make every
            # gradient a sum over ~1e8 (edge, channel) masks, and a pre-activation within rounding of 0 flips its mask
            # between two fp32 summation orders — a discrete jump the CPU-vs-fp64 error does not see)
            assert gpu_err <= max(50.0 * cpu_err, 2e-4 * s, 2e-4 * gmax), (name, k, gpu_err, cpu_err, s, gmax)
    # weights as they are after construction; BatchNorm buffers moved by the one training forward on EVERY side
    ref_model.eval(); model.eval(); m64.eval()
    with torch.no_grad():
        pr, pg_, p64 = ref_model(bc), model(bg), m64(b64)
        mae_ref = float(torch.nn.functional.l1_loss(pr, bc.y))
        mae = float(torch.nn.functional.l1_loss(pg_, bg.y))
        mae64 = float(torch.nn.functional.l1_loss(p64, b64.y))
    _close(pg_, p64, 1e-4, name + " fp32 eval prediction")
    assert abs(mae - mae64) < 1e-5 * max(1.0, abs(mae64)), (name, mae, mae64)
    # bf16 compute mode against the fp32 oracle
    m16 = getattr(models, name)(ds, compute_dtype="bf16", **kw)
    m16.load_state_dict(ref_model.state_dict())
    m16.to(DEV).eval()
    _, bg16 = _batches(ds, ids, torch.bfloat16)
    with torch.no_grad():
        p16 = m16(bg16)
    _close(p16, pr, 5e-2, name + " bf16 eval prediction")
    mae16 = float(torch.nn.functional.l1_loss(p16, bg16.y))
    assert abs(mae16 - mae_ref) < 2e-2 * max(1.0, abs(mae_ref)), (name, mae16, mae_ref)
    m16.train()
    out16 = m16(bg16)
    torch.nn.functional.l1_loss(out16, bg16.y).backward()
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in m16.parameters()), name
    return mae_ref, mae, mae16


# ------------------------------------------------------------------------------------------------ cfg2
@pytest.fixture(scope="module")
def bulk():
    from matdeeplearn_amd.process import synthetic_bulk
    ds = _composition_targets(synthetic_bulk(3072, seed=3))
    assert np.diff(ds.node_ptr).max() > 64                    # graphs wider than the source window are present
    return ds.to(DEV)


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_cfg2_cgconv_kernels_on_bulk_batch(bulk, dtype):
    """K2 / K3 / K3c on a whole bulk-like batch (N ~ 7.8e4, E ~ 1.0e6: >= 4 node groups per backward wave, so the
    dynamic schedule is the one that runs) against the oracle op: forward and every gradient."""
    from matdeeplearn_amd import ops
    ids = np.arange(3072)
    bc, bg = _batches(bulk, ids, dtype)
    assert bg.num_nodes // 32 * 2 >= 4 * 1024                # the condition under which cg_launch goes dynamic
    C, G = 64, 50
    g = torch.Generator().manual_seed(5)
    rnd = lambda *s: torch.randn(*s, generator=g)
    x = rnd(bc.x.shape[0], C).to(dtype).float()
    ea = bc.edge_attr.to(dtype).float()
    k = 3.0 / (2 * C + G) ** 0.5
    wf, ws = (rnd(C, 2 * C + G) * k).to(dtype).float(), (rnd(C, 2 * C + G) * k).to(dtype).float()
    bf, bs = rnd(C) * 0.1, rnd(C) * 0.1
    gout = rnd(bc.x.shape[0], C).to(dtype).float()
    xo, wfo, wso, bfo, bso = [t.clone().requires_grad_(True) for t in (x, wf, ws, bf, bs)]
    ref = oops.cgconv(xo, bc.edge_index, ea, wfo, bfo, wso, bso, "mean")
    (ref * gout).sum().backward()
    xd = x.to(DEV).to(dtype).requires_grad_(True)
    wfd, wsd, bfd, bsd = [t.to(DEV).clone().requires_grad_(True) for t in (wf, ws, bf, bs)]
    out = ops.cgconv(xd, None, bg.edge_attr if dtype == torch.float32 else ea.to(DEV).to(dtype), wfd, bfd, wsd, bsd, "mean", csr=bg.csr)
    (out.float() * gout.to(DEV)).sum().backward()
    tol = 2e-5 if dtype == torch.float32 else 3e-2
    wtol = 1e-4 if dtype == torch.float32 else 3e-2          # weight gradients sum 1e6 edge terms in a different order
    _close(out, ref, tol, "out")
    _close(xd.grad, xo.grad, tol, "dx")
    _close(wfd.grad, wfo.grad, wtol, "dW_f")
    _close(wsd.grad, wso.grad, wtol, "dW_s")
    _close(bfd.grad, bfo.grad, wtol, "db_f")
    _close(bsd.grad, bso.grad, wtol, "db_s")


def test_cfg2_cgcnn_model_fp32_and_bf16(bulk):
    kw = dict(dim1=64, dim2=64, pre_fc_count=1, gc_count=4, post_fc_count=3)
    mae_ref, mae, mae16 = _model_parity("CGCNN", kw, bulk, np.arange(1024))
    assert np.isfinite([mae_ref, mae, mae16]).all()


def test_cfg2_cgcnn_model_split_bf16_meets_the_north_star_tolerance(bulk):
    """compute_dtype="bf16x3" (fp32 storage, the CGConv products on (hi, lo)-split bf16 operands, MDL_SPLIT_BF16) on the cfg2
    workload against the CPU oracle at the same weights: eval prediction to 2e-4 of the prediction scale, |dMAE| < 1e-5
    (north_star's criterion — the bf16 mode misses it by two orders), a finite training step whose loss matches the oracle's,
    and the split form really ran (the prediction differs from the exact-fp32 product's by more than fp32 rounding)."""
    from matdeeplearn_amd import models
    kw = dict(dim1=64, dim2=64, pre_fc_count=1, gc_count=4, post_fc_count=3)
    torch.manual_seed(0)
    ref_model = omodels.CGCNN(bulk, **kw)
    mx3 = models.CGCNN(bulk, compute_dtype="bf16x3", **kw)
    m32 = models.CGCNN(bulk, compute_dtype="fp32", **kw)
    assert mx3.split_products and not m32.split_products and mx3.compute_dtype == torch.float32
    for m in (mx3, m32):
        m.load_state_dict(ref_model.state_dict())
        m.to(DEV)
    bc, bg = _batches(bulk, np.arange(1024))
    ref_model.train(); mx3.train(); m32.train()
    lr = torch.nn.functional.mse_loss(ref_model(bc), bc.y)
    lx = torch.nn.functional.mse_loss(mx3(bg), bg.y)
    torch.nn.functional.mse_loss(m32(bg), bg.y)                 # (moves m32's BatchNorm buffers like the others')
    lx.backward()
    assert abs(float(lx) - float(lr)) < 1e-4 * max(1.0, abs(float(lr)))
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in mx3.parameters())
    ref_model.eval(); mx3.eval(); m32.eval()
    with torch.no_grad():
        pr, px, p32 = ref_model(bc), mx3(bg), m32(bg)
    _close(px, pr, 2e-4, "CGCNN bf16x3 eval prediction")
    mae_ref, mae = float(torch.nn.functional.l1_loss(pr, bc.y)), float(torch.nn.functional.l1_loss(px, bg.y))
    assert abs(mae - mae_ref) < 1e-5 * max(1.0, abs(mae_ref)), (mae, mae_ref)
    d = float((px - p32).abs().max() / p32.abs().max())
    assert d > 1e-7, "the split-product kernels did not run (prediction identical to the exact-fp32 form)"


# ------------------------------------------------------------------------------------------------ cfg3
@pytest.fixture(scope="module")
def mof():
    from matdeeplearn_amd.process import synthetic_mof
    ds = _composition_targets(synthetic_mof(96, seed=4))
    assert np.diff(ds.node_ptr).max() > 200
    return ds.to(DEV)


def test_cfg2_bf16_by_source_sums_train_like_fp32_sums():
    """The default bf16 backward keeps the by-source sums r_src of every CGConv layer in bf16 (packed bf16 atomics: one rounding
    to 8 mantissa bits per window flush / out-of-window add, ops._RSRC16) where the first version accumulated in fp32.  Two
    checks at the training level, both on bulk-like graphs with the headline model (CGCNN 64 x 4):
    (i) the same training — seed, batches, AdamW — with the bf16 sums and with fp32 sums (ops._RSRC16 = False): per-step losses
        within 1 % of each other over the first 10 steps (measured 2e-3), and over all 30 steps a mean drift below 3x that of a
        CONTROL + 2 % — the fp32-sums training run twice: AdamW turns any rounding difference of a near-zero gradient into +-lr
        steps, so two trainings drift apart step by step whatever their arithmetic (measured: 2.8 % mean / 20 % worst step for
        bf16 vs fp32 sums, 2.4 % / 16 % for the control) —, held-out MAE (of a barely trained model: a sanity bound) within 30 % or 3x the control's spread + 5 %;
    (ii) gradient error of dx against the fp32 mode as a function of the node's OUT-degree (the number of terms a source row
        sums): the error of the bf16-sum path, relative to the tensor scale, must not grow with the degree faster than the
        fp32-sum path's does (bound: within 2x of it in every degree bucket, and below 2e-2 everywhere)."""
    from matdeeplearn_amd import models, ops
    from matdeeplearn_amd.process import synthetic_bulk
    from matdeeplearn_amd.training import make_optimizer
    ds = _composition_targets(synthetic_bulk(1024, seed=6)).to(DEV)
    kw = dict(dim1=64, dim2=64, pre_fc_count=1, gc_count=4, post_fc_count=3)
    rng = np.random.default_rng(1)
    batches = [rng.choice(896, size=128, replace=False) for _ in range(30)]
    held = np.arange(896, 1024)
    prev = ops._RSRC16
    curves, maes = {}, {}
    try:
        for tag, flag in (("bf16_sums", True), ("fp32_sums", False), ("fp32_again", False)):
            ops._RSRC16 = flag
            torch.manual_seed(0)
            m = models.CGCNN(ds, compute_dtype="bf16", **kw).to(DEV)
            opt = make_optimizer(m.parameters(), "AdamW", lr=0.002)
            m.train()
            losses = []
            for ids in batches:
                b = ds.collate(ids, edge_dtype=torch.bfloat16, x_dtype=torch.bfloat16)
                opt.zero_grad(set_to_none=True)
                with ops.zero_arena(torch.device(DEV)):
                    loss = torch.nn.functional.l1_loss(m(b), b.y)
                    loss.backward()
                opt.step()
                losses.append(float(loss.detach()))
            curves[tag] = np.array(losses)
            m.eval()
            b = ds.collate(held, edge_dtype=torch.bfloat16, x_dtype=torch.bfloat16)
            with torch.no_grad():
                maes[tag] = float(torch.nn.functional.l1_loss(m(b).float(), b.y))
        a, c, c2 = curves["bf16_sums"], curves["fp32_sums"], curves["fp32_again"]
        rel = np.abs(a - c) / np.maximum(np.abs(c), 1e-6)
        ctl = np.abs(c2 - c) / np.maximum(np.abs(c), 1e-6)            # the same arithmetic twice: drift from atomic order alone
        # measured (tools/dbg/rs16_drift.py): bf16 vs fp32 sums mean 2.8 % / max 20 %, control (fp32 sums twice) 2.4 % / 16 %, first
        # ten steps 2e-3 both: the drift of the bf16 sums is the drift any two runs show
        assert np.isfinite(a).all() and rel[:10].max() < 0.01 and rel.mean() < 3 * ctl.mean() + 0.02 and rel.max() < 0.5, (
            rel.round(4).tolist(), ctl.round(4).tolist(), a.round(3).tolist(), c.round(3).tolist())
        # held-out MAE after 30 steps is that of a barely trained model (BatchNorm running statistics of 30 batches): two runs of
        # the SAME arithmetic differ by several per cent; the bf16 sums must stay within 3x that control + 5 %
        d_ctl = abs(maes["fp32_again"] - maes["fp32_sums"]) / maes["fp32_sums"]
        d_b16 = abs(maes["bf16_sums"] - maes["fp32_sums"]) / maes["fp32_sums"]
        assert d_b16 < 3 * d_ctl + 0.05 or d_b16 < 0.30, (maes, d_b16, d_ctl)      # (a sanity bound: measured 10-14 %, control 2-7 %)
        print("bf16 vs fp32 by-source sums: loss drift mean %.4f max %.4f (control %.4f / %.4f), held-out MAE %s" % (
            rel.mean(), rel.max(), ctl.mean(), ctl.max(), maes))
        # (ii) one CGConv layer, gradient w.r.t. x by out-degree bucket
        n, ei = None, None
        b = ds.collate(np.arange(512), edge_dtype=torch.bfloat16, x_dtype=torch.bfloat16)
        csr, N, C = b.csr, b.num_nodes, 64
        g = torch.Generator().manual_seed(3)
        x0 = torch.randn(N, C, generator=g).to(DEV)
        wf, ws = (torch.randn(C, 2 * C + 50, generator=g) * 0.15).to(DEV), (torch.randn(C, 2 * C + 50, generator=g) * 0.15).to(DEV)
        bf, bs = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        gout = torch.randn(N, C, generator=g).to(DEV)
        ea32 = ops.rbf_expand(torch.rand(csr.E, generator=g).to(DEV))

        def dx(dtype, flag):
            ops._RSRC16 = flag
            # (the bf16 sums through the kernel the headline batch runs — edge-per-lane kernel 2 — whatever this batch's size)
            ops.K3_VARIANT = "edge_lane" if flag else None
            try:
                x = x0.detach().to(dtype).clone().requires_grad_(True)          # (a fresh leaf: .to() of the same dtype returns x0 itself)
                out = ops.cgconv(x, None, ea32.to(dtype), wf, bf, ws, bs, "mean", csr=csr)
                (out.float() * gout).sum().backward()
            finally:
                ops.K3_VARIANT = None
            return x.grad.float()
        ref = dx(torch.float32, False)
        err = {tag: (dx(torch.bfloat16, flag) - ref).abs().max(dim=1).values for tag, flag in (("bf16_sums", True), ("fp32_sums", False))}
        outdeg = torch.bincount(csr.src.long(), minlength=N)
        scale = float(ref.abs().max())
        seen = 0
        for lo, hi in ((1, 8), (8, 12), (12, 16), (16, 24), (24, 10 ** 6)):
            sel = (outdeg >= lo) & (outdeg < hi)
            if int(sel.sum()) < 20:
                continue
            seen += 1
            e16, e32 = float(err["bf16_sums"][sel].mean()) / scale, float(err["fp32_sums"][sel].mean()) / scale
            assert e16 < 2e-2 and e16 <= 2.0 * e32 + 1e-3, ("out-degree [%d, %d)" % (lo, hi), e16, e32)
        assert seen >= 2
    finally:
        ops._RSRC16 = prev


def test_cfg3_schnet_demo_on_mof_like_graphs(mof):
    kw = dict(dim1=100, dim2=100, dim3=150, cutoff=8, pre_fc_count=1, gc_count=4, post_fc_count=3)   # config.yml:162-183
    _model_parity("SchNet", kw, mof, np.arange(64))


def test_cfg3_schnet_interaction_block_bf16(mof):
    """One InteractionBlock (K4 path) in bf16 against the fp32 oracle on bf16-rounded operands: output and the
    gradients w.r.t. x and every parameter, 3e-2 of the tensor scale."""
    from matdeeplearn_amd import nn as pnn
    bc, bg = _batches(mof, np.arange(48), torch.bfloat16)
    torch.manual_seed(2)
    C, F = 100, 150
    ob = oops.InteractionBlock(C, 50, F, 8.0)
    with torch.no_grad():
        for p in ob.parameters():
            p.copy_(p.to(torch.bfloat16).float())
            if p.dim() == 1:
                p.add_(0.05 * torch.randn_like(p)).copy_(p.to(torch.bfloat16).float())
    pb = pnn.InteractionBlock(C, 50, F, 8.0)
    pb.load_state_dict(ob.state_dict())
    pb.to(DEV)
    g = torch.Generator().manual_seed(7)
    x = torch.randn(bc.x.shape[0], C, generator=g).to(torch.bfloat16).float()
    gout = torch.randn(bc.x.shape[0], C, generator=g)
    ea = bc.edge_attr.to(torch.bfloat16).float()
    xo = x.clone().requires_grad_(True)
    ref = ob(xo, bc.edge_index, bc.edge_weight, ea)
    (ref * gout).sum().backward()
    xd = x.to(DEV).to(torch.bfloat16).requires_grad_(True)
    out = pb(xd, None, bg.edge_weight, ea.to(DEV).to(torch.bfloat16), csr=bg.csr)
    (out.float() * gout.to(DEV)).sum().backward()
    _close(out, ref, 3e-2, "InteractionBlock out")
    _close(xd.grad, xo.grad, 3e-2, "dx")
    og = dict(ob.named_parameters())
    for k, p in pb.named_parameters():
        _close(p.grad, og[k].grad, 4e-2, k)


# ------------------------------------------------------------------------------------------------ cfg4
def test_cfg4_megnet_demo_on_bulk_like_graphs(bulk):
    kw = dict(dim1=100, dim2=100, dim3=100, pre_fc_count=1, gc_count=4, gc_fc_count=1, post_fc_count=3)  # config.yml:184-205
    _model_parity("MEGNet", kw, bulk, np.arange(256))


def test_cfg4_megnet_bf16_training_tracks_fp32():
    """cfg4's performance mode must TRAIN like the parity mode, not only evaluate like it at fixed weights: MEGNet_demo
    (config.yml:184-205) on bulk-like graphs, the same seed / batches / AdamW settings in fp32 and in bf16 compute mode,
    24 steps at batch 64.  Stated tolerances: (i) the bf16 loss curve stays within 35 % of the fp32 curve at every step and
    within 8 % on average (observed over a dozen runs: 12-20 % at the worst single step, 2-3 % on average; every step draws a
    fresh 64-graph batch, so the curve is the per-batch loss, and AdamW turns the order noise of fp32 atomics into +-lr steps
    of near-zero-gradient parameters: the worst step moves from run to run); (ii) at the bf16-TRAINED weights the bf16 and
    fp32 compute modes predict the same on held-out graphs to 5 % of max(prediction scale, 0.1 of the target scale) (observed 1 %); (iii) the held-out
    MAE of the two trained models agrees to 15 %.  What is NOT asserted is equality of the two weight sets: AdamW turns rounding noise in near-zero gradients
    (BatchNorm biases) into +-lr steps, so two trainings drift apart in those parameters — in fp32 against fp32 as well."""
    from matdeeplearn_amd import models, ops
    from matdeeplearn_amd.process import synthetic_bulk
    from matdeeplearn_amd.training import make_optimizer
    ds = _composition_targets(synthetic_bulk(512, seed=5)).to(DEV)
    kw = dict(dim1=100, dim2=100, dim3=100, pre_fc_count=1, gc_count=4, gc_fc_count=1, post_fc_count=3)
    rng = np.random.default_rng(0)
    batches = [rng.choice(448, size=64, replace=False) for _ in range(24)]
    held = np.arange(448, 512)
    curves, trained = {}, {}
    for cd, dt in (("fp32", torch.float32), ("bf16", torch.bfloat16)):
        torch.manual_seed(0)
        m = models.MEGNet(ds, compute_dtype=cd, **kw).to(DEV)
        opt = make_optimizer(m.parameters(), "AdamW", lr=0.0005)
        m.train()
        losses = []
        for ids in batches:
            b = ds.collate(ids, edge_dtype=dt, x_dtype=dt)
            opt.zero_grad(set_to_none=True)
            with ops.zero_arena(torch.device(DEV)):
                loss = torch.nn.functional.l1_loss(m(b), b.y)
                loss.backward()
            opt.step()
            losses.append(float(loss.detach()))
        trained[cd] = m
        curves[cd] = np.array(losses)
    f, h = curves["fp32"], curves["bf16"]
    assert np.isfinite(f).all() and np.isfinite(h).all(), (f, h)
    rel = np.abs(h - f) / np.maximum(np.abs(f), 1e-6)
    assert rel.max() < 0.35 and rel.mean() < 0.08, (rel.round(3).tolist(), f.round(3).tolist(), h.round(3).tolist())

    def held_out(weights, cd):
        dt = torch.bfloat16 if cd == "bf16" else torch.float32
        m = models.MEGNet(ds, compute_dtype=cd, **kw).to(DEV)
        m.load_state_dict(trained[weights].state_dict())
        m.eval()
        b = ds.collate(held, edge_dtype=dt, x_dtype=dt)
        with torch.no_grad():
            p = m(b).float()
        return p.cpu(), float(torch.nn.functional.l1_loss(p, b.y.view_as(p)))

    p_bb, mae_b = held_out("bf16", "bf16")
    p_bf, _ = held_out("bf16", "fp32")
    _, mae_f = held_out("fp32", "fp32")
    # 5 % of max(prediction scale, 0.1 of the target scale): after 24 steps at lr 5e-4 the model still predicts nearly the
    # same small number for every graph on some runs (|p| <= 0.015 on standardised targets of scale 1), and 5 % of THAT is less
    # than the bf16 rounding of the O(1) activations behind it (observed there: 1.2e-3 absolute)
    y_scale = float(np.abs(np.asarray(ds.y)).max())           # standardised composition targets: ~2-3
    scale = max(float(p_bf.abs().max()), 0.1 * y_scale)
    err = float((p_bb - p_bf).abs().max())
    assert err <= 5e-2 * scale, ("bf16-trained weights: bf16 vs fp32 compute mode", err, float(p_bf.abs().max()), y_scale)
    assert abs(mae_b - mae_f) < 0.15 * mae_f, (mae_b, mae_f)


def test_cfg4_megnet_edge_block_with_batchnorm_bf16_gradients():
    """Megnet_EdgeModel (K6 first layer + BatchNorm over the EDGE rows + second Linear -> ReLU -> BatchNorm, megnet.py:41-56)
    in bf16 against the fp32 oracle block on bf16-rounded operands and weights: output and the gradients w.r.t. the node
    state, the edge state, u and every parameter (the kernel-level bf16 gradient check of the chain the MEGNet bench leg
    runs).  Tolerances: output 6e-2 of its scale (two bf16 Linear + two bf16 BatchNorm roundings on values of magnitude 5;
    observed 4.9e-2), dx / de / du 5e-2 (observed <= 1e-2), parameter gradients 6e-2 of max(their own scale, 1e-1 of the
    block's largest gradient) — a bias in front of a training-mode BatchNorm has an exactly zero true gradient when its
    ReLU is active, so those tensors are compared against the floor, not against their own ~1e-3 scale (a sum of 2e4 cancelling
    bf16-rounded terms: observed error 2e-3 of the largest gradient)."""
    from matdeeplearn_amd.models.megnet import Megnet_EdgeModel
    bulk = _composition_targets(__import__("matdeeplearn_amd.process", fromlist=["synthetic_bulk"]).synthetic_bulk(96, seed=9)).to(DEV)
    bc, bg = _batches(bulk, np.arange(64), torch.bfloat16)
    d = 64
    torch.manual_seed(3)
    oe = omodels.MegnetEdgeModel(d, "relu", "True", "True", 0.0, 1)
    with torch.no_grad():
        # biases of +2.5 on small weights keep (nearly) every ReLU unit active: a pre-activation within bf16 rounding of the kink
        # flips its mask between the two sides and moves a gradient by a whole upstream value — not a kernel property
        for k_, p_ in oe.named_parameters():
            if "edge_mlp" in k_:
                p_.copy_(((p_ * 0.3) if p_.dim() == 2 else torch.full_like(p_, 2.5) + 0.1 * torch.randn_like(p_)).to(torch.bfloat16).float())
            else:
                p_.copy_((p_ + 0.05 * torch.randn_like(p_)).to(torch.bfloat16).float())
    pe = Megnet_EdgeModel(d, "relu", "True", "True", 0.0, 1)
    pe.load_state_dict(oe.state_dict())
    pe.to(DEV)
    oe.train(); pe.train()
    g = torch.Generator().manual_seed(11)
    N, E, B = bc.x.shape[0], bc.edge_index.shape[1], int(bc.batch.max()) + 1
    r16 = lambda t: t.to(torch.bfloat16).float()
    x, e, u = r16(torch.randn(N, d, generator=g)), r16(torch.randn(E, d, generator=g)), r16(torch.randn(B, d, generator=g))
    row, col = bc.edge_index[0], bc.edge_index[1]
    xo, eo, uo = [t.clone().requires_grad_(True) for t in (x, e, u)]
    ref = oe(xo[row], xo[col], eo, uo, bc.batch[row])
    gout = torch.randn(E, d, generator=g)
    (ref * gout).sum().backward()
    xd, ed, ud = [t.to(DEV).to(torch.bfloat16).requires_grad_(True) for t in (x, e, u)]
    row32, col32 = bg.csr.row, bg.csr.col
    assert pe.fused_ok(xd, ed)
    out = pe.forward_fused(xd, row32, col32, ed, ud, bg.batch)
    assert out.dtype == torch.bfloat16
    (out.float() * gout.to(DEV)).sum().backward()
    _close(out, ref, 6e-2, "edge block out")
    for a, r_, nm in ((xd, xo, "dx"), (ed, eo, "de"), (ud, uo, "du")):
        _close(a.grad, r_.grad, 5e-2, nm)
    og = dict(oe.named_parameters())
    gmax = max(float(v.grad.abs().max()) for v in og.values())
    for k, p_ in pe.named_parameters():
        ref_g = og[k].grad
        err = float((p_.grad.detach().float().cpu() - ref_g).abs().max())
        assert err <= 6e-2 * max(float(ref_g.abs().max()), 1e-1 * gmax), (k, err, float(ref_g.abs().max()), gmax)


# ------------------------------------------------------------------------------------------------ cfg5
@pytest.fixture(scope="module")
def slabs():
    from matdeeplearn_amd.process import synthetic_surface
    return _composition_targets(synthetic_surface(24, seed=8)).to(DEV)


def test_cfg5_mpnn_demo_on_surface_like_slabs(slabs):
    """MPNN_demo (config.yml:141-156: dims 100 / 100 / 100, 4 NNConv + GRU layers) on surface-like slabs, few enough that the
    oracle's literal E x C x C edge tensor fits: fp32 prediction / gradients / val-MAE, then the bf16 compute mode (K7 on
    MFMA, the written-out GRU step) against the same oracle prediction."""
    kw = dict(dim1=100, dim2=100, dim3=100, pre_fc_count=1, gc_count=4, post_fc_count=3)
    _model_parity("MPNN", kw, slabs, np.arange(12))


def test_cfg5_five_model_ensemble_on_surface_like_slabs():
    """The Ensemble driver with all five models on the device (product kernels) against the same driver on the oracle:
    same seed -> same split, same initial weights, same batches; one epoch of fp32 training stays within 2e-3."""
    from matdeeplearn_amd.process import synthetic_surface
    from matdeeplearn_amd.training import train_ensemble
    ds = _composition_targets(synthetic_surface(96, seed=6))
    training = dict(target_index=0, loss="l1_loss", train_ratio=0.7, val_ratio=0.1, test_ratio=0.2, verbosity=0)
    base = dict(dim1=32, dim2=32, dim3=24, pre_fc_count=1, gc_count=2, gc_fc_count=1, post_fc_count=1, epochs=1, lr=0.002,
                batch_size=24, optimizer="AdamW", optimizer_args={}, scheduler="ReduceLROnPlateau",
                scheduler_args={"mode": "min", "factor": 0.8, "patience": 10})
    mps = [dict(base, model=m) for m in ("CGCNN", "SchNet", "MPNN", "MEGNet", "GCN")]
    job = dict(job_name="ens", seed=17, save_model="False", write_output="False")
    quiet = lambda *a: None
    gpu = train_ensemble("cuda", 1, copy.copy(ds).to(DEV), job, training, mps, log=quiet)
    cpu = train_ensemble("cpu", 1, _cpu_twin(ds), job, training, mps, log=quiet,
                         model_factory=lambda n: omodels.REGISTRY[n], rbf=lambda d: oops.rbf_expand(d))
    assert gpu["model_errors"].shape == (5,)
    assert np.allclose(gpu["model_errors"], cpu["model_errors"], rtol=2e-3, atol=2e-3), (gpu["model_errors"], cpu["model_errors"])
    assert abs(gpu["ensemble_error"] - cpu["ensemble_error"]) < 2e-3 * max(1.0, cpu["ensemble_error"])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_full_size_batch_is_the_concatenation_of_its_halves(dtype):
    """Size-independent property at BASELINE's full bench size (8192 bulk-like graphs, ~2.6e6 edges — the oracle would need
    minutes): graphs do not interact inside a conv layer, so K1, K2, K3 / K3c and pooling on the whole batch must equal the
    same operators on its two halves (rows concatenated; weight gradients added).  The full batch runs the backward's
    dynamic group schedule, the halves' tiles and groups fall on other boundaries."""
    from matdeeplearn_amd import ops
    from matdeeplearn_amd.process import synthetic_bulk
    dev = torch.device(DEV)
    ds = synthetic_bulk(8192, seed=0).to(dev)
    ids = np.arange(8192)
    full = ds.collate(ids, edge_dtype=dtype, x_dtype=dtype)
    parts = [ds.collate(ids[:4096], edge_dtype=dtype, x_dtype=dtype), ds.collate(ids[4096:], edge_dtype=dtype, x_dtype=dtype)]
    assert full.num_edges > 2_000_000 and full.num_edges == sum(p.num_edges for p in parts)
    # K1 + batch assembly: row e depends on edge e only -> bit-equal
    assert torch.equal(full.edge_attr, torch.cat([p.edge_attr for p in parts]))
    C = 64
    g = torch.Generator().manual_seed(0)
    x = torch.randn(full.num_nodes, C, generator=g).to(dtype).to(dev)
    wf = (torch.randn(C, 2 * C + 50, generator=g) * 0.1).to(dev)
    ws = (torch.randn(C, 2 * C + 50, generator=g) * 0.1).to(dev)
    bf = (torch.randn(C, generator=g) * 0.1).to(dev)
    bs = (torch.randn(C, generator=g) * 0.1).to(dev)
    go = torch.randn(full.num_nodes, C, generator=g).to(dtype).to(dev)
    n1 = parts[0].num_nodes

    def run(batches, xs, gos):
        outs, gxs, pools = [], [], []
        ps = [t.clone().requires_grad_(True) for t in (wf, bf, ws, bs)]
        for b, xv, gv in zip(batches, xs, gos):
            xv = xv.clone().requires_grad_(True)
            out = ops.cgconv(xv, None, b.edge_attr, ps[0], ps[1], ps[2], ps[3], "mean", csr=b.csr)
            (out.float() * gv.float()).sum().backward()
            outs.append(out.detach()); gxs.append(xv.grad)
            pools.append(ops.global_mean_pool(out.detach(), b.batch, b.num_graphs))
        return torch.cat(outs), torch.cat(gxs), torch.cat(pools), [p.grad for p in ps]

    of, gxf, pf, gwf = run([full], [x], [go])
    oh, gxh, ph, gwh = run(parts, [x[:n1], x[n1:]], [go[:n1], go[n1:]])
    tol = 1e-5 if dtype == torch.float32 else 8e-3          # bf16: one ulp (the tile a row's sum is split over differs)
    _close(of, oh, tol, "K2 output")
    _close(gxf, gxh, tol * 4, "K3 / K3c dx")
    _close(pf, ph, tol, "pooled output")
    for a, b, nm in zip(gwf, gwh, ("dW_f", "db_f", "dW_s", "db_s")):
        _close(a, b, 2e-4 if dtype == torch.float32 else 5e-3, nm)
