"""bf16 CGConv on the device against the fp64 oracle, per row, within ALLOWED times the error of the rounding model
(tests/cgconv_budget.py): forward and all gradients of every kernel family the dispatch of csrc/cgconv.hip (cg_launch) and
ops._CGConvFn can reach at small shapes — among them the bias read from bpack (G % 16 == 0), the generic kernels at vec == 1
and the backward's dynamic group schedule, which no other test runs.  test_cgconv_budget_host.py shows that these checks can
fail: every mutation of the model stands at least 2 x ALLOWED over it."""
import pytest
import torch

import cgconv_budget as B

pytestmark = pytest.mark.gpu


def dev():
    return torch.device("cuda:0")


def _device_run(c):
    """ops.cgconv forward + backward once on the case's inputs in bf16 -> dict like reference64's (CPU tensors)"""
    from matdeeplearn_amd import ops
    d, bf16 = dev(), torch.bfloat16
    i = c["inputs"]
    n = c["n"]
    x = i["x"].to(d).to(bf16).requires_grad_(True)
    ea = i["ea"].to(d).to(bf16).requires_grad_(c["need_de"])
    par = [None if t is None else t.to(d).clone().requires_grad_(True) for t in (i["wf"], i["bf"], i["ws"], i["bs"])]
    ei = i["ei"].to(d)
    csr = ops.build_csr(ei, n, assume_sorted=c["sorted"])
    assert (csr.eperm is None) == c["sorted"]
    out = ops.cgconv(x, ei, ea, par[0], par[1], par[2], par[3], c["aggr"], csr=csr)
    (out.float() * i["gout"].to(d)).sum().backward()
    torch.cuda.synchronize()
    assert out.dtype == bf16 and x.grad.dtype == bf16
    g = lambda t: None if t is None else t.grad.cpu()
    r = dict(out=out.detach().cpu(), dx=x.grad.cpu(), dW_f=g(par[0]), db_f=g(par[1]), dW_s=g(par[2]), db_s=g(par[3]))
    if c["need_de"]:
        assert ea.grad is not None and ea.grad.dtype == bf16
        r["de"] = ea.grad.cpu()
    return r


def _check(name, label="", variant=None, k3=None, det=False, **options):
    """One case under one dispatch: prints the ratios, asserts each <= ALLOWED, restores every switch it touched."""
    from matdeeplearn_amd import ops
    c = B.case(name)
    prev_variant, prev_opts = ops.K3_VARIANT, ops.configure(**options)
    try:
        ops.K3_VARIANT = variant
        with ops.deterministic(det):
            got = _device_run(c)
        if k3 is not None:
            assert ops.last_k3() == k3, "%s %s: backward edge pass %d ran, %d was meant" % (name, label, ops.last_k3(), k3)
    finally:
        ops.K3_VARIANT = prev_variant
        ops.configure(**prev_opts)
    r = B.ratios(got, c["model"], c["ref"])
    assert len(r) == (7 if c["need_de"] else 6) - (0 if c["inputs"]["bf"] is not None else 2)
    print("[budget] %-22s %-14s %s" % (name, label, B.fmt(r)))
    over = {k: v for k, v in r.items() if not v <= B.ALLOWED[k]}
    assert not over, "%s %s: over the budget %s: %s" % (name, label, {k: B.ALLOWED[k] for k in over}, over)
    return r


@pytest.mark.parametrize("label,kw", [
    ("per_wave", dict(variant="per_wave", k3=1)),
    ("edge_lane", dict(variant="edge_lane", k3=2)),
    ("deterministic", dict(det=True, k3=3)),
    ("rsrc16_off", dict(variant="per_wave", k3=1, rsrc16=False)),
])
def test_static_64(label, kw):
    """C 64, G 50, n 200: the static kernels; every backward edge pass (per-wave, edge-per-lane, deterministic shape), fp32
    by-source sums."""
    _check("static64", label, **kw)


@pytest.mark.parametrize("variant,k3", [("per_wave", 1), ("edge_lane", 2)])
def test_far_sources(variant, k3):
    """n 700, sources up to +-400 nodes from their target: by-source sums outside the 64-row register window (per-edge atomics)"""
    _check("far_sources", variant, variant=variant, k3=k3)


@pytest.mark.parametrize("name", ["partial_group", "single_node"])
def test_partial_group_and_single_node(name):
    """n 33: one full 32-node group plus one node; n 1: a single node"""
    _check(name)


def test_static_32():
    """C 32: the 32-channel static kernels and the K3c node kernel at 32 channels"""
    _check("static32", k3=1)


@pytest.mark.parametrize("name,label,options", [("wide128", "", {}), ("wide100", "pad128", {"pad128": True}),
                                                ("wide100", "no_pad128", {"pad128": False})])
def test_wide(name, label, options):
    """C 128, and C 100 on zero-padded rows (static 128-channel kernels) or at its own width (generic kernels, one channel slice
    of the packed weights per workgroup)"""
    _check(name, label, **options)


@pytest.mark.parametrize("name", ["bpack_64_64", "bpack_64_48_no_bias", "bpack_32_16"])
def test_bias_from_bpack(name):
    """G % 16 == 0: no zero-padding K column is free, the bias seeds the accumulators from bpack (bias_col == 0) — forward,
    backward edge pass; one case without biases (bpack is zeros, no bias gradient)"""
    c = B.case(name)
    assert c["G"] % 16 == 0 and (c["inputs"]["bf"] is None) == (name == "bpack_64_48_no_bias")
    _check(name)


@pytest.mark.parametrize("name", ["generic_20_7", "generic_30_7", "generic_64_41"])
def test_generic_kernels(name):
    """run-time shapes: C 20 (8-byte row vectors), C 30 (vec == 1: element loads), G 7 / 41 (odd: two-byte staging words, EW 1) and
    C 64 with G 41"""
    _check(name)


def test_sparse_graph_takes_the_dynamic_group_schedule():
    """N 2000, most nodes isolated, E < N: the backward hands out 32-node groups from a counter, the last ones as half groups.
    The launch arithmetic of cg_launch (csrc/cgconv.hip) for this shape is restated here so that the case keeps meaning it."""
    c = B.case("sparse")
    N, E = c["n"], c["inputs"]["ei"].shape[1]
    NS, waves = 2, 4
    grid = -(-(max(1, min(-(-E // 128), N)) * NS) // waves)
    while (grid * waves) % NS:
        grid += 1
    n_groups = -(-N // 32)
    assert n_groups * NS >= 4 * grid * waves, "dynamic schedule not taken at N = %d, E = %d" % (N, E)
    assert 0 < n_groups - 2 * (grid * waves // NS) < n_groups, "no half-group tail"
    _check("sparse", k3=1)


def test_sum_aggregation():
    _check("sum", k3=1)


def test_unsorted_edge_list():
    """a shuffled edge list: the CSR carries an edge permutation, the kernels read a target-sorted copy of the edge features"""
    _check("unsorted")


@pytest.mark.parametrize("name", ["de_static64", "de_bpack_64_64"])
def test_edge_attr_gradient(name):
    """edge_attr.requires_grad: mdl_cgconv_bwd_edge with its general epilogue, rows = edges; G 64 reads the bias from bpack"""
    _check(name)
