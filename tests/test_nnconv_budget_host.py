"""The error budget of tests/nnconv_budget.py, checked without a GPU: the graph holds what it promises, the mirror of K7's
dispatch puts every case on the route it is named after, the rounding models are sane stand-ins for the bf16 kernels and the bf16
layer, every mutation of them (a kernel bug in miniature) breaks the budget that test_gpu_nnconv_budget.py enforces, and the
re-associated fp64 reference of the largest layer case equals the oracle's NNConv."""
import pytest
import torch

import nnconv_budget as B


def _scale_err(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def _close_4e2(a, ref):
    """close(a, b, 4e-2, 4e-2) of tests/test_gpu_kernels.test_nnconv_contraction_matches_oracle"""
    a, ref = a.detach().float(), ref.detach().float()
    return torch.allclose(a, ref, rtol=4e-2, atol=4e-2 * (float(ref.abs().max()) + 1e-30))


# ---------------------------------------------------------------------------------------------
# graph
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,kw", [(100, {}), (100, {"sort": False}), (100, {"by_source": True}), (1100, {}), (1100, {"max_in": 3})])
def test_nn_graph_contains_what_it_promises(n, kw):
    for seed in range(4):
        ei, probe, hub33, hub100, zeros = B.nn_graph(n, seed=seed, **kw)
        ckw = {k: v for k, v in kw.items() if k != "by_source"}
        base = B.cf_graph(n, seed=seed, **ckw)[0]
        indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
        # three nodes without out-edges: the first, the last, one inner node that is neither a hub nor a special-degree node
        assert zeros[0] == 0 and zeros[2] == n - 1 and 0 < zeros[1] < n - 1
        assert [int(outdeg[z]) for z in zeros] == [0, 0, 0]
        assert zeros[1] not in (hub33, hub100) and int(indeg[zeros[1]]) not in B.SPECIAL_DEGREES
        assert int(indeg[zeros[1]]) >= 1, "the inner node still receives messages"
        # ... which cf_graph alone does not give at n = 100 (as generated, every node there is a source)
        if n == 100 and not kw:
            assert int((torch.bincount(base[0], minlength=n)[1:n - 1] == 0).sum()) == 0
        # the hubs are untouched: exactly 33 and 100 out-edges (one 32-edge chunk + 1, three chunks + a ragged one)
        assert int(outdeg[hub33]) == 33 and int(outdeg[hub100]) == 100 and B.HUB_OUT_DEGREES == (100, 33)
        # only sources were redirected: same edge count, every target where it was, every in-degree budget_graph's
        assert ei.shape == base.shape
        if not kw.get("by_source"):
            assert torch.equal(ei[1], base[1])
            moved = (ei[0] != base[0]).nonzero().flatten()
            assert moved.numel() >= 1 and set(base[0][moved].tolist()) <= set(zeros)
            assert not set(ei[0][moved].tolist()) & {hub33, hub100, *zeros}, "handed to a source that is not a hub"
            assert int((ei[0][moved] - base[0][moved]).abs().max()) <= 3, "... and a neighbouring one"
        assert torch.equal(indeg, torch.bincount(B.budget_graph(n, seed=seed, **dict(ckw, sort=True))[0][1], minlength=n))
        assert indeg[0] == 0 and indeg[n - 1] == 0 and indeg[probe] == B.PROBE_DEGREE
        for deg in B.SPECIAL_DEGREES:
            assert int((indeg == deg).sum()) >= 1
        assert bool((ei[0] == ei[1]).any()), "self loops"
        assert int(ei.min()) >= 0 and int(ei.max()) < n
        by_target = bool((ei[1][1:] >= ei[1][:-1]).all())
        by_source = bool((ei[0][1:] >= ei[0][:-1]).all())
        assert by_source == bool(kw.get("by_source")) and by_target == (kw.get("sort", True) and not kw.get("by_source"))
        rowptr_s, eid_s = B.by_source_csr(ei, n)
        assert rowptr_s.dtype == torch.int32 and int(rowptr_s[-1]) == ei.shape[1]
        assert torch.equal(rowptr_s[1:] - rowptr_s[:-1], outdeg.to(torch.int32))
        assert torch.equal(torch.sort(eid_s).values, torch.arange(ei.shape[1], dtype=torch.int32))
        assert by_source == torch.equal(eid_s, torch.arange(ei.shape[1], dtype=torch.int32))
        s_sorted = ei[0][eid_s.long()]
        assert bool((s_sorted[1:] >= s_sorted[:-1]).all())


# ---------------------------------------------------------------------------------------------
# dispatch mirror
# ---------------------------------------------------------------------------------------------
ROUTES = {   # the table of the cases: (kind, forward flat, backward flat, backward instantiation)
    "w100": ("mfma", True, True, 5), "at_small_limit": ("mfma", True, True, 5), "over_small_limit": ("mfma", True, True, 7),
    "full_budget": ("mfma", True, True, 7), "too_big": ("mfma", False, False, 7), "odd_bytes": ("mfma", False, False, 7),
    "overrun30": ("mfma", True, True, 5), "smallest_flat": ("mfma", True, True, 5), "d3_two": ("mfma", False, False, 7),
    "y_misaligned": ("mfma", False, False, 7), "dy_misaligned": ("mfma", True, False, 7), "by_source_null": ("mfma", True, True, 5),
    "scalar_odd": ("scalar", False, False, 0), "scalar_wide_co": ("scalar", False, False, 0),
    "scalar_wide_d3": ("scalar", False, False, 0),
}
SHAPES = {
    "w100": (100, 100), "at_small_limit": (128, 80), "over_small_limit": (104, 100), "full_budget": (128, 112),
    "too_big": (128, 128), "odd_bytes": (30, 34), "overrun30": (34, 20), "smallest_flat": (2, 4), "d3_two": (4, 2),
    "y_misaligned": (100, 100), "dy_misaligned": (100, 100), "by_source_null": (100, 100), "scalar_odd": (25, 33),
    "scalar_wide_co": (130, 100), "scalar_wide_d3": (24, 130),
}


def test_every_case_is_pinned_to_its_route():
    assert list(B.OP_CASES) == list(ROUTES) == list(SHAPES)
    for name, (Co, D3, route, kw) in B.OP_CASES.items():
        assert (Co, D3) == SHAPES[name] and route == ROUTES[name], name
        assert B.k7_route(Co, D3, kw.get("y_off", 0) % 16, kw.get("dy_off", 0) % 16) == route, name
        c = B.op_case(name)
        assert (c["eid_s"] is None) == (name == "by_source_null") and (c["y_off"], c["dy_off"]) == (kw.get("y_off", 0), kw.get("dy_off", 0))
    assert B.OP_CASES["y_misaligned"][3] == {"y_off": 4} and B.OP_CASES["dy_misaligned"][3] == {"dy_off": 4}
    # what the names say, in the terms of csrc/nnconv.hip
    assert 128 * 80 == 256 * 5 * 8 and 104 * 100 > 256 * 5 * 8 and 104 * 100 % 8 == 0           # the <5> / <7> boundary
    assert 128 * 112 == 256 * 7 * 8 == B.K7_CHUNK_BUDGET and 128 * 128 > B.K7_CHUNK_BUDGET       # the chunk budget
    assert (30 * 34 * 2) % 16 != 0 and (34 + 15) // 16 * 16 == 48                                # odd_bytes: k padded 34 -> 48
    assert 64 - 34 == 30 and (34 * 20 * 2) % 16 == 0                                             # overrun30: rows 34..63 of the second block
    assert 2 * 4 * 2 == 16                                                                       # smallest_flat: one chunk
    assert 130 * 100 > 48 * 256 and 25 * 33 <= 48 * 256 and 24 * 130 <= 48 * 256                 # RMAX = 48: the second pass
    # the boundaries of the mirror itself
    assert B.k7_route(128, 128) == ("mfma", False, False, 7) and B.k7_route(130, 128)[0] == "scalar" and B.k7_route(2, 2)[0] == "mfma"
    assert B.k7_route(100, 100, 8, 0) == ("mfma", False, False, 7) and B.k7_route(100, 100, 0, 8) == ("mfma", True, False, 7)
    assert (50 * 98 * 2) % 16 == 8 and B.k7_route(50, 98) == ("mfma", False, False, 7)           # blocks that do not end on a 16-byte boundary
    # every LDS requirement of nn_check holds (the scalar kernels stage Y_j as fp32 with a padded row)
    for Co, D3 in SHAPES.values():
        assert (Co * (D3 + 1) + D3 + Co) * 4 <= 160 * 1024


def test_allowed_is_within_its_limits():
    assert set(B.ALLOWED) == set(B.TENSORS) == set(B.OP_TENSORS) | set(B.LAYER_TENSORS)
    assert all(2.0 <= v <= 5.0 for v in B.ALLOWED.values()), B.ALLOWED


# ---------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.OP_CASES))
def test_op_model_is_sane(name):
    c = B.op_case(name)
    i, Co, D3 = c["inputs"], c["Co"], c["D3"]
    for k in ("Y", "h", "dm"):
        assert torch.equal(B.bfr(i[k]), i[k]), (name, k)                    # exact in bf16
    assert float(i["h"].min()) == 0.0 and 0.3 < float((i["h"] == 0).float().mean()) < 0.7, "h is post-ReLU"
    assert i["Y"].shape == (c["n"], Co * D3) and i["h"].shape == (c["E"], D3) and i["dm"].shape == (c["E"], Co)
    for k in B.OP_TENSORS:
        err = _scale_err(c["model"][k], c["ref"][k])
        print("%s %s: model error %.2e of scale" % (name, k, err))
        assert 0.0 < err < 4e-2 and _close_4e2(c["model"][k], c["ref"][k]), (name, k, err)
    assert B.op_ratios(c["model"], c["model"], c["ref"], Co, D3) == pytest.approx({k: 1.0 for k in B.OP_TENSORS})
    for z in c["zeros"]:
        assert float(c["ref"]["dY"][z].abs().max()) == 0.0 and float(c["model"]["dY"][z].abs().max()) == 0.0
    assert B.op_rows("dY", c["model"]["dY"], Co, D3).shape == (c["n"] * Co, D3)


@pytest.mark.parametrize("name,mutation", [(n, m) for n in B.OP_CASES for m in B.MUTATIONS])
def test_every_op_mutation_breaks_the_budget(name, mutation):
    """A condition, not a measurement: on the inputs of every op-level case, each mutation stands at least 2 x ALLOWED over the
    model on the tensor of the kernel it models, and leaves the other two tensors alone."""
    c = B.op_case(name)
    r = B.op_ratios(B.op_mutated(name, mutation), c["model"], c["ref"], c["Co"], c["D3"])
    (own,) = B.MUTATIONS[mutation][1]
    print("%s / %s: %s at %.1fx (allowed %.1f)   all: %s" % (name, mutation, own, r[own], B.ALLOWED[own], B.fmt(r)))
    assert r[own] >= 2.0 * B.ALLOWED[own], (name, mutation, r)
    for k in set(B.OP_TENSORS) - {own}:
        assert r[k] == pytest.approx(1.0), (mutation, k)


# ---------------------------------------------------------------------------------------------
# layer level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.LAYER_CASES))
def test_layer_model_is_sane(name):
    c = B.layer_case(name)
    i = c["inputs"]
    for k in ("x", "ea", "w1", "w2", "wr", "gout"):
        assert torch.equal(B.bfr(i[k]), i[k]), (name, k)
    for k in ("b1", "b2", "b"):
        assert not torch.equal(B.bfr(i[k]), i[k]) and float(i[k].abs().min()) > 0, "biases are general fp32 and non-zero"
    assert (name in B.REASSOCIATED) == (name == "layer_wide_100")
    for k in B.LAYER_TENSORS:
        err = _scale_err(c["model"][k], c["ref"][k])
        print("%s %s: model error %.2e of scale" % (name, k, err))
        assert 0.0 < err < 4e-2 and _close_4e2(c["model"][k], c["ref"][k]), (name, k, err)
    assert B.layer_ratios(c["model"], c["model"], c["ref"]) == pytest.approx({k: 1.0 for k in B.LAYER_TENSORS})


def test_layer_cases_are_what_their_names_say():
    shape = lambda name: B.wide_launch_shape(*[B.layer_case(name)[k] for k in ("n", "Ci", "Co", "D3")])
    assert shape("layer_small") [0] is False and shape("layer_add")[0] is False
    assert shape("layer_wide_24") == (True, 64, 4, 96) and 24 * 28 == 672
    assert shape("layer_wide_100") == (True, 128, 53, 16)
    assert 3000 < B.layer_case("layer_wide_100")["E"] < 4000
    assert B.layer_case("layer_add")["aggr"] == "add" and B.LAYER_CASES["layer_add"][:4] == B.LAYER_CASES["layer_small"][:4]
    for name in B.LAYER_CASES:
        c = B.layer_case(name)
        assert B.k7_route(c["Co"], c["D3"]) [0] == "mfma" and c["probes"][0] is not None


@pytest.mark.parametrize("name,mutation", [(n, m) for n in B.LAYER_CASES for m in B.LAYER_MUTATIONS
                                           if B.layer_applies(m, B.LAYER_CASES[n][4])])
def test_every_layer_mutation_breaks_the_budget(name, mutation):
    """the same condition on the layer: the witness is a tensor the mutated pass writes; every other tensor is left alone"""
    c = B.layer_case(name)
    r = B.layer_ratios(B.layer_mutated(name, mutation), c["model"], c["ref"])
    own = B.LAYER_MUTATIONS[mutation][1]
    witness = max(own, key=lambda k: r[k] / B.ALLOWED[k])
    print("%s / %s: witness %s at %.1fx (allowed %.1f)   all: %s" % (name, mutation, witness, r[witness], B.ALLOWED[witness], B.fmt(r)))
    assert r[witness] >= 2.0 * B.ALLOWED[witness], (name, mutation, r)
    for k in set(B.LAYER_TENSORS) - set(own):
        assert r[k] == pytest.approx(1.0), (mutation, k)


def test_mean_divisor_mutation_does_not_apply_to_add():
    assert [m for m in B.LAYER_MUTATIONS if not B.layer_applies(m, "add")] == ["mean_divisor_off_by_one"]
    assert all(B.layer_applies(m, "mean") for m in B.LAYER_MUTATIONS)


def test_reassociated_reference_equals_the_oracle():
    """layer_wide_100 takes its fp64 reference in the re-associated form: on layer_small (mean) and layer_add that form equals
    oracle.ops.NNConv(...).double(), which builds the E x Ci x Co tensor, to 1e-12 of each tensor's largest element"""
    for name in ("layer_small", "layer_add"):
        c = B.layer_case(name)
        re = B.layer_reassociated64(aggr=c["aggr"], **c["inputs"])
        for k in B.LAYER_TENSORS:
            assert re[k].dtype == torch.float64 and re[k].shape == c["ref"][k].shape
            assert _scale_err(re[k], c["ref"][k]) < 1e-12, (name, k)


@pytest.mark.parametrize("mutation", ["mean_divisor_off_by_one", "edge_dropped_forward", "edge_dropped_backward"])
def test_the_old_bound_does_not_see_these_layer_bugs(mutation):
    """Why the layer level exists: at the workload's widths (layer_wide_100) a mean divisor that is off by one, an edge missing
    from the forward and an edge missing from the backward all pass close(a, ref, 4e-2, 4e-2) on every one of the eight tensors,
    while the budget sees each of them at least 2 x ALLOWED over the model."""
    c = B.layer_case("layer_wide_100")
    mutant = B.layer_mutated("layer_wide_100", mutation)
    for k in B.LAYER_TENSORS:
        assert _close_4e2(mutant[k], c["ref"][k]), (mutation, k)
    r = B.layer_ratios(mutant, c["model"], c["ref"])
    assert max(r[k] / B.ALLOWED[k] for k in B.LAYER_MUTATIONS[mutation][1]) >= 2.0, r
