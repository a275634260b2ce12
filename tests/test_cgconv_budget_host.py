"""The error budget of tests/cgconv_budget.py, checked without a GPU: the rounding model is a sane stand-in for the bf16 kernels,
every mutation of it (a kernel bug in miniature) breaks the budget that test_gpu_cgconv_budget.py enforces, and the two most
plausible of them pass the 3e-2-of-scale bound of the older parity tests — which is why the budget exists."""
import pytest
import torch

import cgconv_budget as B

PROBED = [k for k in B.CASES if B.CASES[k][0] >= 9 and "sparse" not in B.CASES[k][3]]
UNPROBED = [k for k in B.CASES if k not in PROBED]


def _scale_err(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def _close_3e2(a, ref):
    """close(a, b, 3e-2, 3e-2) of tests/test_gpu_kernels.py"""
    a, ref = a.detach().float(), ref.detach().float()
    return torch.allclose(a, ref, rtol=3e-2, atol=3e-2 * (float(ref.abs().max()) + 1e-30))


def test_budget_graph_contains_what_it_promises():
    for n, kw in ((200, {}), (700, {"window": 400}), (33, {}), (65, {}), (200, {"sort": False})):
        ei, probe = B.budget_graph(n, seed=3, **kw)
        deg = torch.bincount(ei[1], minlength=n)
        assert deg[0] == 0 and deg[n - 1] == 0, "first and last node are isolated"
        assert deg[probe] == B.PROBE_DEGREE
        for d in B.SPECIAL_DEGREES:
            assert int((deg == d).sum()) >= 1, "no node of in-degree %d at n = %d" % (d, n)
        assert bool((ei[0] == ei[1]).any()), "self loops"
        assert int(ei.min()) >= 0 and int(ei.max()) < n
        is_sorted = bool((ei[1][1:] >= ei[1][:-1]).all())
        assert is_sorted == kw.get("sort", True)
    ei, probe = B.budget_graph(1)
    assert probe is None and ei.shape[1] == 5 and int(ei.max()) == 0
    ei = B.sparse_graph(2000, 200, seed=1)
    assert int((torch.bincount(ei[1], minlength=2000) == 0).sum()) >= 1700 and 1000 <= ei.shape[1] <= 1900


def test_allowed_is_within_its_limits():
    assert set(B.ALLOWED) == set(B.TENSORS)
    assert all(2.0 <= v <= 5.0 for v in B.ALLOWED.values()), B.ALLOWED


def test_row_ratio_definition():
    ref = torch.zeros(4, 8, dtype=torch.float64)
    model = torch.zeros(4, 8)
    model[0] += 1.0
    model[1] += 2.0
    model[2] += 4.0                                          # row errors 1, 2, 4, 0: median (lower of the middle two) = 1
    got = torch.zeros(4, 8)
    got[3] += 3.0                                            # a row where the model is exact: floored at the median
    got[2] += 2.0
    assert B.row_ratio(got, model, ref) == pytest.approx(3.0)
    assert B.row_ratio(torch.full((8,), 2.0), torch.full((8,), 0.5), torch.zeros(8, dtype=torch.float64)) == pytest.approx(4.0)


@pytest.mark.parametrize("name", PROBED)
def test_rounding_model_is_sane(name):
    """The model is not the reference (it rounds) and is well inside the old 3e-2-of-scale bound on every tensor."""
    c = B.case(name)
    for k, ref in c["ref"].items():
        if ref is None:
            assert c["model"][k] is None
            continue
        err = _scale_err(c["model"][k], ref)
        print("%s %s: model error %.2e of scale" % (name, k, err))
        assert 0.0 < err < 3e-2, (name, k, err)
        assert _close_3e2(c["model"][k], ref), (name, k)
    assert B.ratios(c["model"], c["model"], c["ref"]) == pytest.approx({k: 1.0 for k in c["ref"] if c["ref"][k] is not None})


# (mean aggregation has a divisor to get wrong; sum aggregation has none, so that pair does not exist)
_PAIRS = [(n, m) for n in PROBED for m in B.MUTATIONS if not (m == "degree_off_by_one" and B.CASES[n][4] != "mean")]


@pytest.mark.parametrize("name,mutation", _PAIRS)
def test_every_mutation_breaks_the_budget(name, mutation):
    """A condition, not a measurement: on the inputs of every GPU case that has the probe node, each mutation stands at least
    2 x ALLOWED over the model on at least one tensor (the witness).  Cases without the probe (the single node, the sparse
    graph) are exempt: there is no degree-13 node to mutate."""
    c = B.case(name)
    r = B.ratios(B.mutated(name, mutation), c["model"], c["ref"])
    witness = max(r, key=lambda k: r[k] / B.ALLOWED[k])
    print("%s / %s: witness %s at %.1fx (allowed %.1f)   all: %s" % (name, mutation, witness, r[witness], B.ALLOWED[witness], B.fmt(r)))
    assert r[witness] >= 2.0 * B.ALLOWED[witness], (name, mutation, r)


def test_unprobed_cases_are_exempt_from_the_sensitivity_condition():
    assert sorted(UNPROBED) == ["single_node", "sparse"]
    for name in UNPROBED:
        assert B.case(name)["probe"] is None


@pytest.mark.parametrize("name", ["static64", "static32"])
@pytest.mark.parametrize("mutation", ["edge_dropped_forward", "edge_dropped_backward", "degree_off_by_one"])
def test_the_old_bound_does_not_see_a_dropped_edge_or_a_wrong_divisor(name, mutation):
    """Why this file exists: the mutated model still passes close(a, b, 3e-2, 3e-2) on the four weight and bias gradients."""
    c = B.case(name)
    mutant = B.mutated(name, mutation)
    for k in ("dW_f", "db_f", "dW_s", "db_s"):
        assert _close_3e2(mutant[k], c["ref"][k]), (name, mutation, k)
