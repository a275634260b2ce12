"""The fused Set2Set readout (csrc/set2set.hip through ops.set2set / nn.Set2Set) on the device.

Truth is the fp64 oracle.ops.set2set_loop (test_set2set_host.loop_reference: the same loop, graphs without nodes included).  The error
criterion is the one of test_gpu_model.py: for the output and every gradient the device error against fp64 may be at most
max(20 x the error of the fp32 CPU oracle.ops.Set2Set on the same inputs, 2e-4 x the largest fp64 entry)."""
import copy
import functools
import math
import os

import numpy as np
import pytest
import torch

import test_gpu_model as tgm
from oracle import ops as oops
from test_set2set_host import loop_reference, lstm_params, segments

pytestmark = pytest.mark.gpu
SIZES = [1, 2, 13, 64, 65, 300, 0, 1000]         # one node, an empty graph in the middle, graphs far longer than a wave holds
NAMES = ("out", "dx", "dw_ih", "dw_hh", "db_ih", "db_hh")


def dev():
    return torch.device("cuda:0")


# ---------------------------------------------------------------------------------------------
# references (computed once per shape, never modified)
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _inputs(C, bf16, x_scale):
    B, batch = len(SIZES), segments(SIZES)
    gen = torch.Generator().manual_seed(100 + C)
    x = torch.randn(sum(SIZES), C, generator=gen) * x_scale
    if bf16:
        x = x.bfloat16().float()                                        # the oracle is fed the bf16-rounded values
    gout = torch.randn(B, 2 * C, generator=gen)
    return x, batch, B, gout, tuple(lstm_params(C, 7 + C, torch.float32))


def _oracle_module(C, T, params, dtype):
    m = oops.Set2Set(C, processing_steps=T).to(dtype)
    with torch.no_grad():
        for p, v in zip((m.lstm.weight_ih_l0, m.lstm.weight_hh_l0, m.lstm.bias_ih_l0, m.lstm.bias_hh_l0), params):
            p.copy_(v)
    return m


@functools.lru_cache(maxsize=None)
def _references(C, T, bf16=False, x_scale=1.0):
    """(fp64 truth, fp32 CPU oracle) as dicts out / dx / dw_ih / dw_hh / db_ih / db_hh"""
    x, batch, B, gout, params = _inputs(C, bf16, x_scale)
    x64 = x.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in params]
    out = loop_reference(x64, batch, B, *p64, T)
    g = torch.autograd.grad((out * gout.double()).sum(), [x64] + p64)
    truth = dict(zip(NAMES, [out.detach()] + list(g)))
    m = _oracle_module(C, T, params, torch.float32)
    x32 = x.clone().requires_grad_(True)
    o32 = m(x32, batch)
    assert o32.shape[0] == B
    g32 = torch.autograd.grad((o32 * gout).sum(), [x32] + list(m.lstm.parameters()))
    cpu = dict(zip(NAMES, [o32.detach()] + list(g32)))
    return truth, cpu


def _device_run(C, T, bf16=False, x_scale=1.0, x_grad=True, no_grad=False):
    from matdeeplearn_amd import ops
    x, batch, B, gout, params = _inputs(C, bf16, x_scale)
    xd = x.to(dev()).to(torch.bfloat16 if bf16 else torch.float32).requires_grad_(x_grad and not no_grad)
    pd = [p.to(dev()).requires_grad_(not no_grad) for p in params]
    si = ops._seg_index(batch.to(dev()), B, True)
    if no_grad:
        with torch.no_grad():
            return dict(out=ops.set2set(xd, si, *pd, T))
    out = ops.set2set(xd, si, *pd, T)
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, 2 * C)
    g = torch.autograd.grad((out * gout.to(dev())).sum(), ([xd] if x_grad else []) + pd)
    res = dict(zip(NAMES if x_grad else (NAMES[:1] + NAMES[2:]), [out.detach()] + list(g)))
    torch.cuda.synchronize()
    return res


def _bf16_ulp(v):
    return 2.0 ** (math.floor(math.log2(v)) - 7)


def _check(got, truth, cpu, bf16=False, tag=None):
    for k in NAMES:
        t, g, c = truth[k], got[k].detach().cpu().double(), cpu[k].double()
        assert torch.isfinite(g).all(), (tag, k)
        scale = float(t.abs().max())
        floor = 2e-4 * scale
        if bf16 and k == "dx":
            assert got[k].dtype == torch.bfloat16
            t = t.bfloat16().double()                                  # the device stores dx in x's dtype: compare rounded values
            floor = max(floor, _bf16_ulp(scale))
        err_cpu = float((c - truth[k]).abs().max())
        err_gpu = float((g - t).abs().max())
        print(tag, k, "gpu", err_gpu, "cpu32", err_cpu, "scale", scale)
        assert err_gpu <= max(20.0 * err_cpu, floor), (tag, k, err_gpu, err_cpu, scale)


# ---------------------------------------------------------------------------------------------
# operator against fp64
# ---------------------------------------------------------------------------------------------
SHAPES = [(1, 3), (24, 3), (32, 3), (64, 3), (100, 3), (128, 3), (32, 1), (32, 8)]


@pytest.mark.parametrize("C,T", SHAPES)
def test_fp32_output_and_gradients_match_the_fp64_loop(C, T):
    truth, cpu = _references(C, T)
    got = _device_run(C, T)
    _check(got, truth, cpu, tag=("fp32", C, T))
    # the graph without nodes: r = 0, q finite; the one-node graph: r = x
    assert float(got["out"][6, C:].abs().max()) == 0.0 and torch.isfinite(got["out"][6]).all()
    x = _inputs(C, False, 1.0)[0]
    assert torch.equal(got["out"][0, C:].cpu(), x[0])


@pytest.mark.parametrize("C,T", SHAPES)
def test_bf16_rows_match_the_fp64_loop_on_the_rounded_values(C, T):
    truth, cpu = _references(C, T, bf16=True)
    got = _device_run(C, T, bf16=True)
    _check(got, truth, cpu, bf16=True, tag=("bf16", C, T))


@pytest.mark.parametrize("bf16", [False, True])
def test_scores_spanning_hundreds_stay_finite_and_exact(bf16):
    """x scaled by 30 at C = 64: the scores of one graph span hundreds — exp(e) without the maximum subtracted overflows"""
    C, T = 64, 3
    truth, cpu = _references(C, T, bf16=bf16, x_scale=30.0)
    x, batch, B, gout, params = _inputs(C, bf16, 30.0)
    m = _oracle_module(C, T, params, torch.float64)
    with torch.no_grad():
        q_last = m(x.double(), batch)[:, :C]
    span = float(((x.double() * q_last[batch]).sum(1)).abs().max())
    assert span > 100.0, span                                           # (the case is what it claims to be)
    got = _device_run(C, T, bf16=bf16, x_scale=30.0)
    assert torch.isfinite(got["out"]).all()
    _check(got, truth, cpu, bf16=bf16, tag=("range", bf16))


# ---------------------------------------------------------------------------------------------
# rows outside every segment, repeatability, forward without saved state
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_rows_outside_every_segment_are_invisible_and_get_zero_gradients(dtype):
    from matdeeplearn_amd import ops
    C, T, PAD = 32, 3, 40
    x, batch, B, gout, params = _inputs(C, False, 1.0)
    N = x.shape[0]
    rowptr = torch.tensor([0] + list(np.cumsum(SIZES)), dtype=torch.int32, device=dev())
    seg = torch.cat([batch, torch.full((PAD,), B, dtype=torch.int64)]).to(torch.int32).to(dev())
    pd = [p.to(dev()).requires_grad_(True) for p in params]
    go = gout.to(dev())

    def run(xt, si):
        xt = xt.to(dev()).to(dtype).requires_grad_(True)
        out = ops.set2set(xt, si, *pd, T)
        return [out.detach()] + list(torch.autograd.grad((out * go).sum(), [xt] + pd))

    ref = run(x, ops._seg_index(batch.to(dev()), B, True))
    for fill in (0.0, 1e30):
        xp = torch.cat([x, torch.full((PAD, C), fill)])
        got = run(xp, ops.make_seg_index(rowptr, seg, partial=True))
        assert torch.equal(got[0], ref[0]), fill
        assert got[1].shape[0] == N + PAD and float(got[1][N:].float().abs().max()) == 0.0, fill
        assert torch.equal(got[1][:N], ref[1]), fill
        for a, b in zip(got[2:], ref[2:]):
            assert torch.equal(a, b), fill


def test_two_calls_give_the_same_bits_with_and_without_deterministic_mode():
    from matdeeplearn_amd import ops
    for C, bf16 in ((64, False), (100, True)):
        a, b = _device_run(C, 3, bf16=bf16), _device_run(C, 3, bf16=bf16)
        with ops.deterministic():
            c = _device_run(C, 3, bf16=bf16)
        for k in NAMES:
            assert torch.equal(a[k], b[k]), (C, k)
            assert torch.equal(a[k], c[k]), (C, k, "deterministic")


def test_forward_without_saved_state_and_without_dx_gives_the_same_bits():
    for C, bf16 in ((32, False), (100, True), (1, False)):
        full = _device_run(C, 3, bf16=bf16)
        assert torch.equal(_device_run(C, 3, bf16=bf16, no_grad=True)["out"], full["out"]), C
        nodx = _device_run(C, 3, bf16=bf16, x_grad=False)
        assert "dx" not in nodx
        for k in nodx:
            assert torch.equal(nodx[k], full[k]), (C, k)


# ---------------------------------------------------------------------------------------------
# dispatch: which library calls a readout makes
# ---------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self, real, names):
        self._real, self._names = real, names

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapped(*a):
            self._names.append(name)
            return fn(*a)
        return wrapped


def record(fn):
    """names of the library calls fn() makes (the cached library handle is replaced by a recording proxy for the call)"""
    from matdeeplearn_amd import _lib
    real, names = _lib.lib(), []
    torch.cuda.synchronize()
    _lib._lib = _Recorder(real, names)
    try:
        fn()
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    return names


def _module_step(C, num_layers=1, T=3):
    """(run, result) — run() does forward + backward of nn.Set2Set on the test batch and fills result"""
    from matdeeplearn_amd import nn as mnn
    x, batch, B, gout, _ = _inputs(32, False, 1.0)
    if C != 32:
        x = torch.randn(x.shape[0], C, generator=torch.Generator().manual_seed(C))
        gout = torch.randn(B, 2 * C, generator=torch.Generator().manual_seed(C + 1))
    torch.manual_seed(11)
    m = mnn.Set2Set(C, processing_steps=T, num_layers=num_layers).to(dev())
    xd, bd, go = x.to(dev()).requires_grad_(True), batch.to(dev()), gout.to(dev())
    res = {}

    def run():
        m.zero_grad()
        xd.grad = None
        out = m(xd, bd, B)
        (out * go).sum().backward()
        res.update(out=out.detach(), dx=xd.grad.clone(), dw_ih=m.lstm.weight_ih_l0.grad.clone(), dw_hh=m.lstm.weight_hh_l0.grad.clone(),
                   db_ih=m.lstm.bias_ih_l0.grad.clone(), db_hh=m.lstm.bias_hh_l0.grad.clone())
    return run, res, m


def _is_composed(names):
    return ("mdl_set2set_fwd" not in names and "mdl_set2set_bwd" not in names and names.count("mdl_segment_reduce_fwd") >= 9
            and "mdl_gather_rows" in names)


def test_two_layers_an_unsupported_width_and_the_option_off_take_the_composed_path():
    from matdeeplearn_amd import ops
    run, res, m = _module_step(32, num_layers=2)
    assert not m.fused_path()
    assert _is_composed(record(run)) and tuple(res["out"].shape) == (len(SIZES), 64)
    run, res, m = _module_step(129)
    assert not m.fused_path()
    assert _is_composed(record(run)) and tuple(res["out"].shape) == (len(SIZES), 258)
    run, res, m = _module_step(32)
    assert m.fused_path()
    prev = ops.configure(set2set_fused=False)
    try:
        assert not m.fused_path()
        names = record(run)
    finally:
        ops.configure(**prev)
    assert _is_composed(names)


def test_fused_path_is_one_launch_per_direction():
    run, res, m = _module_step(32)
    run()                                                               # (the segment index of this batch tensor is cached now)
    names = record(run)
    print(names)
    assert [n for n in names if n in ("mdl_set2set_fwd", "mdl_set2set_bwd")] == ["mdl_set2set_fwd", "mdl_set2set_bwd"], names
    assert not [n for n in names if n.startswith("mdl_segment_reduce") or n == "mdl_gather_rows"], names


def test_fused_and_composed_paths_agree_within_the_fp64_criterion():
    from matdeeplearn_amd import ops
    C, T = 32, 3
    run, res, m = _module_step(C)
    x, batch, B, gout, _ = _inputs(C, False, 1.0)
    params = [p.detach().cpu() for p in (m.lstm.weight_ih_l0, m.lstm.weight_hh_l0, m.lstm.bias_ih_l0, m.lstm.bias_hh_l0)]
    x64 = x.double().requires_grad_(True)
    p64 = [p.double().requires_grad_(True) for p in params]
    out = loop_reference(x64, batch, B, *p64, T)
    truth = dict(zip(NAMES, [out.detach()] + list(torch.autograd.grad((out * gout.double()).sum(), [x64] + p64))))
    mo = _oracle_module(C, T, params, torch.float32)
    x32 = x.clone().requires_grad_(True)
    o32 = mo(x32, batch)
    cpu = dict(zip(NAMES, [o32.detach()] + list(torch.autograd.grad((o32 * gout).sum(), [x32] + list(mo.lstm.parameters())))))
    run()
    fused = {k: v.clone() for k, v in res.items()}
    prev = ops.configure(set2set_fused=False)
    try:
        run()
    finally:
        ops.configure(**prev)
    composed = {k: v.clone() for k, v in res.items()}
    _check(fused, truth, cpu, tag="fused")
    _check(composed, truth, cpu, tag="composed")
    for k in NAMES:
        scale = float(truth[k].abs().max())
        err_cpu = float((cpu[k].double() - truth[k]).abs().max())
        diff = float((fused[k].double() - composed[k].double()).abs().max())
        assert diff <= max(20.0 * err_cpu, 2e-4 * scale), (k, diff, err_cpu, scale)


# ---------------------------------------------------------------------------------------------
# models: prediction and gradients against the oracle model, bounds of test_gpu_model.py
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,kw,readouts", [
    ("CGCNN", dict(dim1=32, dim2=32, gc_count=2, post_fc_count=1, pool="set2set"), 1),
    ("CGCNN", dict(dim1=32, dim2=32, gc_count=1, post_fc_count=1, pool="set2set", pool_order="late"), 1),
    ("MEGNet", dict(dim1=32, dim2=32, dim3=24, gc_count=1, gc_fc_count=1, post_fc_count=1, pool="set2set"), 2),
])
def test_models_with_the_fused_readout_match_the_oracle(name, kw, readouts):
    names = record(lambda: tgm.test_other_models_fp32_match_oracle(name, kw))
    assert names.count("mdl_set2set_fwd") == readouts and names.count("mdl_set2set_bwd") == readouts, names


# ---------------------------------------------------------------------------------------------
# graph replay
# ---------------------------------------------------------------------------------------------
def _pt10(n):
    from matdeeplearn_amd.process import from_structures
    z = np.load(os.path.join(tgm.G_DIR, "pt10_dataset.npz"))
    structs = [dict(positions=z["positions"][s], numbers=z["numbers"][s], cell=z["cell"][s], pbc=z["pbc"][s]) for s in range(n)]
    return from_structures(structs, z["y"][:n], [str(v) for v in z["ids"][:n]])


S2S_KW = dict(dim1=32, dim2=32, gc_count=2, post_fc_count=1, pool="set2set")


def test_auto_mode_replays_a_set2set_model_on_the_fused_path_only():
    from matdeeplearn_amd import models, nn as mnn, ops
    from matdeeplearn_amd.process import DeviceLoader
    from matdeeplearn_amd.training.driver import graph_replay_wanted
    ds = _pt10(64).to(dev())
    loader = DeviceLoader(ds, np.arange(64), 16, shuffle=True, seed=1)
    model = models.CGCNN(ds, **S2S_KW).to(dev())
    args = ("auto", ds, model, loader, None, False, "AdamW", "l1_loss")
    assert graph_replay_wanted(*args) is True
    prev = ops.configure(set2set_fused=False)
    try:
        assert graph_replay_wanted(*args) is False
    finally:
        ops.configure(**prev)
    model.set2set = mnn.Set2Set(model.set2set.in_channels, processing_steps=3, num_layers=2).to(dev())
    assert graph_replay_wanted(*args) is False


def test_replayed_steps_of_a_set2set_model_match_the_eager_steps():
    """protocol and bounds of test_gpu_training.test_graph_replayed_step_matches_the_eager_step (fp32 leg: losses to 2e-4, every
    state_dict entry to 5 x 2e-4 of its largest value), three steps of batch 16 on Pt10, deterministic kernels"""
    from matdeeplearn_amd import models, ops
    from matdeeplearn_amd.training import GraphedStep, make_optimizer
    ds = _pt10(64).to(dev())
    B, tol = 16, 2e-4
    rng = np.random.default_rng(0)
    batches = [rng.choice(len(ds), size=B, replace=False) for _ in range(3)]
    with ops.deterministic():
        torch.manual_seed(3)
        m_e = models.CGCNN(ds, compute_dtype="fp32", **S2S_KW).to(dev())
        m_g = copy.deepcopy(m_e)
        o_e = make_optimizer(m_e.parameters(), "AdamW", lr=0.002)
        o_g = make_optimizer(m_g.parameters(), "AdamW", lr=0.002, capturable=True)
        gs = GraphedStep(ds, m_g, o_g, B, compute_dtype=torch.float32)
        m_e.train()
        losses_e, losses_g = [], []
        for ids in batches:
            batch = ds.collate(ids, edge_dtype=torch.float32, x_dtype=torch.float32)
            o_e.zero_grad(set_to_none=True)
            with ops.zero_arena(dev()):
                loss = torch.nn.functional.l1_loss(m_e(batch), batch.y)
                loss.backward()
            o_e.step()
            losses_e.append(float(loss))
            assert gs.step(ids) == (batch.num_edges, batch.num_nodes)
            losses_g.append(float(gs.loss_value))
    assert gs.replays == len(batches) and gs.eager_steps == 0
    print("losses", losses_g, losses_e)
    assert np.allclose(losses_g, losses_e, rtol=tol, atol=tol), (losses_g, losses_e)
    sd_e, sd_g = m_e.state_dict(), m_g.state_dict()
    assert any(k.startswith("set2set.lstm.") for k in sd_e)
    for k in sd_e:
        a, b = sd_g[k].float(), sd_e[k].float()
        assert float((a - b).abs().max()) <= tol * (float(b.abs().max()) + 1e-3) * 5, k
