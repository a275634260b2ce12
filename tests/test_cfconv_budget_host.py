"""The error budget of tests/cfconv_budget.py, checked without a GPU: the graphs hold what they promise, the rounding model is a
sane stand-in for the bf16 CFConv kernels, every mutation of it (a kernel bug in miniature) breaks the budget that
test_gpu_cfconv_budget.py enforces on a tensor of the kernel it models, and a dropped edge in the weight-gradient pass goes
through the 3e-2-of-scale bound of the older parity tests — which is why the budget exists."""
import pytest
import torch

import cfconv_budget as B

PROBED = [k for k in B.CASES if k not in B.EXEMPT]


def _scale_err(a, ref):
    a, ref = a.detach().double(), ref.detach().double()
    return float((a - ref).abs().max() / (ref.abs().max() + 1e-30))


def _close_3e2(a, ref):
    """close(a, b, 3e-2, 3e-2) of tests/test_gpu_kernels.py / BF16_TOL of tests/test_gpu_forces.py"""
    a, ref = a.detach().float(), ref.detach().float()
    return torch.allclose(a, ref, rtol=3e-2, atol=3e-2 * (float(ref.abs().max()) + 1e-30))


def test_cf_graph_contains_what_it_promises():
    for n, kw in ((100, {}), (65, {}), (700, {"window": 400}), (200, {"sort": False}), (3140, {"max_in": 40})):
        ei, probe, hub = B.cf_graph(n, seed=3, **kw)
        indeg, outdeg = torch.bincount(ei[1], minlength=n), torch.bincount(ei[0], minlength=n)
        assert indeg[0] == 0 and indeg[n - 1] == 0, "first and last node are isolated"
        assert indeg[probe] == B.PROBE_DEGREE
        for d in B.SPECIAL_DEGREES:
            assert int((indeg == d).sum()) >= 1, "no node of in-degree %d at n = %d" % (d, n)
        assert outdeg[hub] == 33 and int((outdeg == 100).sum()) >= 1, "hub sources of out-degree 33 and 100"
        assert hub != probe and bool((ei[0] == ei[1]).any()), "self loops"
        assert int(ei.min()) >= 0 and int(ei.max()) < n
        assert bool((ei[1][1:] >= ei[1][:-1]).all()) == kw.get("sort", True)
        # the hubs only took over sources: every in-degree is budget_graph's
        assert torch.equal(indeg, torch.bincount(B.budget_graph(n, seed=3, **dict(kw, sort=True))[0][1], minlength=n))
    ei, probe, hub = B.cf_graph(1)
    assert probe is None and hub is None and ei.shape[1] == 5 and int(ei.max()) == 0


def test_cases_are_what_their_names_say():
    assert tuple(B.CASES["width%d" % F][1] for F in B.WIDTHS) == B.WIDTHS
    for name in B.CASES:
        c, i = B.case(name), B.case(name)["inputs"]
        for k in ("h", "gout", "rbf", "w1", "w2"):                  # exact in bf16 where the layer stores bf16
            assert torch.equal(B.bfr(i[k]), i[k]), (name, k)
        assert float(i["b1"].abs().min()) > 0 and float(i["b2"].abs().min()) > 0, "biases are non-zero"
        lo = float(i["cut"].min())
        assert (lo == 0.0 and int((i["cut"] == 0).sum()) == 7) if name == "small_cutoffs" else 0.5 <= lo, (name, lo)
        assert float(i["cut"].max()) <= 1.0 and c["sorted"] == (name != "unsorted")
    assert B.case("two_groups_plus_one")["n"] == 2 * 32 + 1
    assert B.case("single_node")["n"] == 1 and B.case("single_node")["E"] == 5
    far = B.case("far_sources")["inputs"]["ei"]
    assert int((far[0] - far[1]).abs().max()) > 64


def test_long_case_reaches_the_second_k4d_tile_and_the_steady_state_of_k4b():
    """every K4b workgroup runs at least 3 tiles (interval A / B with `more`, request_rows(tile + 2 G) inside the loop), every
    K4d wave at least 2 (the LDS rbf tile reused behind wave_lds_fence at the loop top)"""
    E = B.case("long")["E"]
    assert 49152 < E < 70000, E
    k4b, k4d = B.long_launch_shape(E)
    assert k4b >= 3 and k4d >= 2, (E, k4b, k4d)
    assert B.long_launch_shape(49152) == (3, 1) and B.long_launch_shape(32768) == (2, 1) and B.long_launch_shape(65536) == (4, 2)


def test_widths_cover_every_tail_shift_of_the_last_block():
    """sh0 / sh1 of csrc/cfconv.hip (the h[src] tail of the last 32-unit block, read 16 bytes at min(u0, F - 8)) recomputed for
    WIDTHS: every shift 0 .. 4 occurs, the last block is empty at 64 / 96 / 128 and two units wide at 66 / 130"""
    seen, per_width = set(), {}
    for F in B.WIDTHS:
        nbk = (F + 2 + 31) // 32
        assert F % 2 == 0 and 64 <= F <= 158 and 32 * (nbk - 1) <= F <= 32 * nbk - 2
        sh = []
        for t in range(2):
            U0 = 32 * (nbk - 1) + 16 * t
            sh += [min(4, (U0 - min(U0, F - 8)) >> 1), min(4, (U0 + 8 - min(U0 + 8, F - 8)) >> 1)]
        per_width[F] = sh
        seen |= set(sh)
    assert seen == {0, 1, 2, 3, 4}, per_width
    assert {(F + 2 + 31) // 32 for F in B.WIDTHS} == {3, 4, 5}
    assert all(per_width[F] == [4, 4, 4, 4] for F in (64, 96, 128)) and all(per_width[F] == [3, 4, 4, 4] for F in (66, 130))
    assert {F % 8 for F in B.WIDTHS} == {0, 2, 4, 6}


def test_allowed_is_within_its_limits():
    assert set(B.ALLOWED) == set(B.TENSORS)
    assert all(2.0 <= v <= 5.0 for v in B.ALLOWED.values()), B.ALLOWED


def test_tile_rows():
    v = torch.arange(70, dtype=torch.float32)
    order = torch.randperm(70, generator=torch.Generator().manual_seed(0))
    rows = B.tile_rows(v, order)
    assert rows.shape == (3, 32) and torch.equal(rows[0], v.double()[order[:32]])
    assert float(rows[2].pow(2).mean()) == pytest.approx(float(v.double()[order[64:]].pow(2).mean()))


@pytest.mark.parametrize("name", list(B.CASES))
def test_rounding_model_is_sane(name):
    """The model is not the reference (it rounds) and is well inside the old 3e-2-of-scale bound on every tensor; the
    stored-activation route differs from the recomputing one in dh alone."""
    c = B.case(name)
    m, ms, mr = B.model(name, "edge"), B.model(name, "stored"), B.model(name, "recompute")
    for k in B.TENSORS + ("a1", "w"):
        err = _scale_err(m[k], c["ref"][k])
        print("%s %s: model error %.2e of scale" % (name, k, err))
        assert 0.0 < err < 3e-2, (name, k, err)
        assert _close_3e2(m[k], c["ref"][k]), (name, k)
    assert B.ratios(m, m, c["ref"], c["order"]) == pytest.approx({k: 1.0 for k in B.TENSORS})
    assert set(ms) == set(mr) == set(m) - {"drbf", "dcut", "dd"}
    for k in mr:
        assert torch.equal(mr[k], m[k]), k
        assert torch.equal(ms[k], m[k]) == (k != "dh"), k
    assert 0.0 < _scale_err(ms["dh"], c["ref"]["dh"]) < 3e-2


_PAIRS = [(n, m) for n in PROBED for m in B.MUTATIONS if B.applies(m, B.CASES[n][1])]


@pytest.mark.parametrize("name,mutation", _PAIRS)
def test_every_mutation_breaks_the_budget(name, mutation):
    """A condition, not a measurement: on the inputs of every probed GPU case, each mutation stands at least 2 x ALLOWED over
    the model on at least one tensor OF THE KERNEL IT MODELS (the witness), and leaves every tensor of the other kernels alone."""
    c = B.case(name)
    r = B.ratios(B.mutated(name, mutation), B.model(name), c["ref"], c["order"])
    own = B.MUTATIONS[mutation][1]
    witness = max(own, key=lambda k: r[k] / B.ALLOWED[k])
    print("%s / %s: witness %s at %.1fx (allowed %.1f)   all: %s" % (name, mutation, witness, r[witness], B.ALLOWED[witness], B.fmt(r)))
    assert r[witness] >= 2.0 * B.ALLOWED[witness], (name, mutation, r)
    for k in set(B.TENSORS) - set(own):
        assert r[k] == pytest.approx(1.0), (mutation, k)


def test_exempt_cases_are_exempt_from_the_sensitivity_condition():
    """no probe node; a dropped edge may carry a cutoff factor near zero; one edge in 68 000 is below the noise of dW"""
    assert sorted(B.EXEMPT) == ["long", "single_node", "small_cutoffs"]
    assert B.case("single_node")["probes"] == (None, None)
    assert sorted(PROBED) == sorted(["width%d" % F for F in B.WIDTHS] + ["two_groups_plus_one", "far_sources", "padded", "unsorted"])
    assert all(B.applies(m, 150) for m in B.MUTATIONS) and not B.applies("tail_piece_shifted", 64)
    assert sum(B.applies("tail_piece_shifted", F) for F in B.WIDTHS) == 7


@pytest.mark.parametrize("F", [150, 94])
def test_the_old_bound_does_not_see_an_edge_dropped_from_the_weight_gradient_pass(F):
    """Why this file exists: with one edge of the probe left out of K4b the model still passes close(a, ref, 3e-2, 3e-2) on all
    four tensors the bug damages (n 400, E about 4 700: the smallest graph of this kind at which it does so at both widths),
    while the budget sees it 10 to 30 times over.
    The other two mutants the budget was meant to be contrasted with do NOT pass the old bound on graphs of this kind, whatever
    their size: measured (largest error beyond 3e-2 |ref|, in units of the tensor's largest element, to be compared with 3e-2)
    tile_dropped_weight_grad 0.08 - 0.14 at E 4 700, 0.06 - 0.12 at E 8 100, 0.02 - 0.05 at E 68 000 (dW1 alone passes there);
    tail_piece_shifted 0.18 - 0.20 on `out` at E 4 700, 0.05 - 0.13 at E 8 100, 0.10 at E 68 000: six units of a degree-13 row
    replaced by their neighbours are a full-size error on those elements, which no bound of 3 % of the largest element lets
    pass.  The old bound is blind to the single edge, not to these."""
    n = 400
    ei, probe, hub = B.cf_graph(n, seed=F)
    inp = B.cf_inputs(ei, n, F, B.G, seed=F)
    ref, order = B.reference64(**inp), B.csr_order(ei)
    model = B.rounding_model(route="recompute", **inp)
    mutant = B.rounding_model(route="recompute", mutation="edge_dropped_weight_grad", probes=(probe, hub), **inp)
    for k in B.K4B:
        assert _close_3e2(mutant[k], ref[k]), (F, k)
    r = B.ratios(mutant, model, ref, order, B.K4B)
    print("F %d: %s" % (F, B.fmt(r)))
    assert max(r[k] / B.ALLOWED[k] for k in B.K4B) >= 2.0, r
