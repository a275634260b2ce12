"""The error budget of tests/head_budget.py, checked without a GPU: the mirrors of the dispatches put every case on the route it
is named after and reach every instantiation of csrc/mlp.hip, csrc/gru.hip and csrc/loss.hip, the integer cases are what they claim,
the rounding model stays inside every derived bound, and every mutation of it (a kernel bug in miniature) breaks what
test_gpu_head_budget.py enforces."""
import os
import re
import types

import pytest
import torch

import head_budget as B

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "matdeeplearn_amd", "csrc")
T = 64 * 72 * 2                                                      # one LDS tile: 64 rows of 72 bf16

# derived by hand from csrc/mlp.hip: (forward, backward), each (tiles, grid, trips, LDS bytes, gy staging)
_REF = ((2, 2, 1, 6 * T, None), (2, 2, 1, 10 * T, "odd"))
_N1 = ((1, 1, 1, 4 * T, None), (1, 1, 1, 6 * T, "even"))
_C3 = ((5, 5, 1, 5 * T, None), (5, 5, 1, 8 * T, "odd"))
MLP_ROUTES = {
    "ref_batch": _REF, "ref_batch_f32io": (_REF[0], (2, 2, 1, 10 * T, "f32")), "no_bias_mix": _REF,
    "n1": _N1, "n63": _N1, "n64": _N1, "n65": ((2, 2, 1, 4 * T, None), (2, 2, 1, 6 * T, "even")),
    "n129": ((3, 3, 1, 4 * T, None), (3, 3, 1, 6 * T, "even")),
    "narrow": ((5, 5, 1, 5 * T, None), (5, 5, 1, 8 * T, "even")), "tiny": ((3, 3, 1, 4 * T, None), (3, 3, 1, 6 * T, "odd")),
    "ragged_widths": ((4, 4, 1, 5 * T, None), (4, 4, 1, 8 * T, "odd")),
    "one_layer_40": ((5, 5, 1, 3 * T, None), (5, 5, 1, 4 * T, "even")), "one_layer_1": ((5, 5, 1, 3 * T, None), (5, 5, 1, 4 * T, "odd")),
    "four_layers": ((5, 5, 1, 6 * T, None), (5, 5, 1, 10 * T, "even")),
    "cancel": _C3, "dead": _C3, "det": (_C3[0], (5, 1, 5, 8 * T, "odd")),
    "trip2_fwd_int": ((514, 512, 2, 6 * T, None), (514, 256, 3, 10 * T, "odd")),
    "trip2_bwd_int": ((258, 258, 1, 6 * T, None), (258, 256, 2, 10 * T, "odd")),
    "trip2_bwd_int_det": ((258, 258, 1, 6 * T, None), (258, 1, 258, 10 * T, "odd")),
}
# derived by hand from csrc/gru.hip, per shape: (forward, backward), each (W, grid, trips)
_V9, _S65 = ((4, 9, 1), (4, 9, 1)), ((1, 65, 1), (1, 65, 1))
GRU_ROUTES = {
    "v4_100": ((4, 26, 1), (4, 26, 1)), "v4_4": ((4, 1, 1), (4, 1, 1)), "s_7": ((1, 1, 1), (1, 1, 1)), "s_30": ((1, 16, 1), (1, 16, 1)),
    "trip2_v4": ((4, 2048, 2), (4, 2048, 2)), "trip2_s": ((1, 2048, 2), (1, 2048, 2)), "saturated": _V9, "zero_state": ((4, 3, 1), (4, 3, 1)),
    "misaligned_gi": _S65, "misaligned_h": _S65, "misaligned_glp": ((4, 17, 1), (1, 65, 1)),
    "g_h_only": _V9, "g_lp_only": _V9, "no_out_lp": _V9,
}
GRU_INSTANCES = {(k, t, w) for k in ("gru_gates_fwd_kernel", "gru_gates_bwd_kernel") for t in ("bf16", "f32") for w in (4, 1)}


def test_every_case_is_pinned_to_its_route():
    assert set(B.MLP_CASES) == set(MLP_ROUTES)
    for name, c in B.MLP_CASES.items():
        assert B.mlp_case_routes(c) == MLP_ROUTES[name], (name, B.mlp_case_routes(c))
        assert B.mlp_case_routes(c)[1][3] <= 160 * 1024, "LDS of one CDNA4 workgroup"
    assert {n.rsplit("_", 1)[0] for n in B.GRU_CASES} == set(GRU_ROUTES)
    for name, c in B.GRU_CASES.items():
        assert B.gru_case_routes(c) == GRU_ROUTES[name.rsplit("_", 1)[0]], (name, B.gru_case_routes(c))
    assert B.MLP_CASES["det"]["det"] and MLP_ROUTES["det"][1][1] == 1
    # the second trips are what they claim
    assert B.MLP_CASES["trip2_fwd_int"]["N"] == 512 * 64 + 65 and B.MLP_CASES["trip2_bwd_int"]["N"] == 256 * 64 + 65
    assert 8193 * 64 == 524352 > 2048 * 256 and 10487 * 50 > 2048 * 256
    # ragged_widths: gy one bf16 past a 4-byte boundary, odd width 3; the loss shapes: the tail, ties, integers
    assert B.MLP_CASES["ragged_widths"]["gy_off"] == 1 and B.MLP_CASES["ragged_widths"]["M"][-1] == 3
    assert {c["n"] for c in B.LOSS_SHAPES.values()} >= {1, 63, 64, 65, 1023, 1024, 1025, 8193}
    assert {c["n_total"] - c["n"] for c in B.LOSS_SHAPES.values()} >= {1, 1024, 3000}
    assert {c["kind"] for c in B.LOSS_CASES.values()} == {0, 1} and len(B.LOSS_CASES) == 2 * len(B.LOSS_SHAPES)


def test_every_instantiation_is_reached():
    """a condition, not a measurement: the launch sites of the three files are pinned, so a new one cannot arrive without a case"""
    gru = set().union(*(B.gru_instances(c) for c in B.GRU_CASES.values()))
    assert gru == GRU_INSTANCES, (GRU_INSTANCES - gru, gru - GRU_INSTANCES)
    sites = {f: len(re.findall(r"hipLaunchKernelGGL\(", open(os.path.join(CSRC, f)).read())) for f in ("mlp.hip", "gru.hip", "loss.hip")}
    assert sites == {"mlp.hip": 2, "gru.hip": len(GRU_INSTANCES), "loss.hip": 2}, sites
    # mlp.hip: one forward and one backward kernel; every case runs both; the staging paths of gy and fp32 I/O are all taken
    assert {MLP_ROUTES[n][1][4] for n in MLP_ROUTES} == {"even", "odd", "f32"}
    assert {len(c["M"]) for c in B.MLP_CASES.values()} == {1, 2, 3, 4}
    # loss.hip: both entry points, both kinds
    assert any(c["n_total"] > c["n"] for c in B.LOSS_CASES.values()) and any(c["n_total"] == c["n"] for c in B.LOSS_CASES.values())


def test_the_mirrors_at_the_edges_of_every_branch():
    r = B.mlp_route
    assert [r(n, 64, (64, 1), False, False, "fwd")[1:3] for n in (64, 65, 512 * 64, 512 * 64 + 1, 1024 * 64 + 1)] == [(1, 1), (2, 1), (512, 1), (512, 2), (512, 3)]
    assert [r(n, 64, (64, 1), False, False, "bwd")[1:3] for n in (256 * 64, 256 * 64 + 1)] == [(256, 1), (256, 2)]
    assert r(10 ** 6, 64, (64, 1), False, True, "bwd")[1:3] == (1, 15625) and r(10 ** 6, 64, (64, 1), False, True, "fwd")[1] == 512
    assert r(5, 64, (64, 3), True, False, "bwd")[4] == "f32" and r(5, 64, (64, 4), False, False, "bwd")[4] == "even"
    g = lambda N, C, dt, lp, f32: B.gru_route(N, C, dt, dict(lp=lp, f32=f32))
    assert g(10, 64, "bf16", (0, 8, None), (0, 16)) == (4, 1, 1) and g(10, 64, "bf16", (0, 4, None), (0, 16))[0] == 1
    assert g(10, 64, "f32", (0, 8, None), (0, 0))[0] == 1 and g(10, 64, "f32", (0, 16, 32), (0, 0))[0] == 4
    assert g(10, 64, "bf16", (0, 0, 0), (0, 8))[0] == 1 and g(10, 64, "bf16", (0, 0, 0), (4, 0))[0] == 1 and g(10, 66, "bf16", (0, 0, 0), (0, 0))[0] == 1
    assert g(10, 64, "bf16", (0, 0, 0, 0, 0), (0, 0, None))[0] == 4 and g(10, 64, "bf16", (0, 0, None, 0, 0), (0, 0, 4))[0] == 1
    assert [g(n, 256, "f32", (0,), (0,))[1:] for n in (4, 5, 8192, 8193)] == [(1, 1), (2, 1), (2048, 1), (2048, 2)]
    with pytest.raises(AssertionError):
        g(1, 0, "f32", (0,), (0,))


def _accept_calls():
    """(keywords of mlp_accepts, expected code) for everything the two entry points refuse, and what they take"""
    ok = dict(N=5, K0=64, M=(64, 2))
    both = [(dict(ok), B.OK), (dict(ok, N=0), B.OK), (dict(ok, N=0, x=None), B.OK), (dict(ok, M=()), B.E_ARG), (dict(ok, M=(2,) * 5), B.E_ARG),
            (dict(ok, K0=63), B.E_UNSUPP), (dict(ok, K0=66), B.E_UNSUPP), (dict(ok, K0=0), B.E_UNSUPP), (dict(ok, M=(63, 2)), B.E_UNSUPP),
            (dict(ok, M=(64, 65)), B.E_UNSUPP), (dict(ok, M=(65, 2)), B.E_UNSUPP), (dict(ok, M=(64, 0)), B.E_UNSUPP), (dict(ok, M=(64, 63)), B.OK),
            (dict(ok, w=[0, None]), B.E_ARG), (dict(ok, w=[2, 0]), B.E_ARG), (dict(ok, x=2), B.E_ARG), (dict(ok, x=None), B.E_ARG),
            (dict(ok, dtype="f32"), B.E_UNSUPP), (dict(ok, N=-1), B.E_ARG), (dict(ok, arrays=False), B.E_ARG),
            (dict(ok, M=(65, 2), w=[None, 0]), B.E_UNSUPP),           # (the width is looked at before the weight of the same layer)
            (dict(ok, M=(64, 65), w=[None, 0]), B.E_ARG)]            # (and layer 0's weight before layer 1's width)
    fwd = [(dict(ok, h=[0, None]), B.E_ARG), (dict(ok, h=[2, 2]), B.OK)]
    bwd = [(dict(ok, gy=None), B.E_ARG), (dict(ok, gy=2), B.E_ARG), (dict(ok, M=(64, 3), gy=2), B.OK), (dict(ok, M=(64, 3), gy=1), B.E_ARG),
           (dict(ok, M=(64, 3), gy=2, f32io=True), B.E_ARG), (dict(ok, M=(64, 3), gy=4, f32io=True), B.OK),
           (dict(ok, dw=[0, None]), B.E_ARG), (dict(ok, h=[None, None]), B.E_ARG), (dict(ok, h=[2, None]), B.E_ARG), (dict(ok, h=[0, None]), B.OK)]
    return [("fwd", k, rc) for k, rc in both + fwd] + [("bwd", k, rc) for k, rc in both + bwd]


def test_mlp_accepts_restates_the_argument_checks():
    for direction, kw, rc in _accept_calls():
        assert B.mlp_accepts(direction, **kw) == rc, (direction, kw)


def test_mlp_head_ok_is_true_only_where_the_entry_points_accept():
    """ops.mlp_head_ok itself, called with CPU stand-ins that carry the attributes it reads (a device tensor cannot exist here):
    wherever it says yes, mlp_accepts takes both directions; head_ok of head_budget.py restates it on plain numbers and the two
    agree on every combination"""
    from matdeeplearn_amd import ops
    n_yes = 0
    for dtype in (torch.bfloat16, torch.float32):
        for N in (0, 1, 300):
            for K0 in (0, 2, 50, 63, 64, 66):
                for addr in (0, 2, 4):
                    for widths in ((1,), (40,), (64, 1), (63, 1), (64, 65), (64, 0), (0,), (34, 62, 3), (64, 64, 64, 64), (2, 2, 2, 2, 2), ()):
                        for rg in (True, False):
                            x = types.SimpleNamespace(dtype=dtype, is_cuda=True, dim=lambda: 2, is_contiguous=lambda: True,
                                                      shape=(N, K0), data_ptr=lambda a=addr: 4096 + a)
                            ks = (K0,) + widths[:-1]
                            lins = [types.SimpleNamespace(in_features=k, out_features=m, weight=types.SimpleNamespace(requires_grad=rg))
                                    for k, m in zip(ks, widths)]
                            yes = bool(ops.mlp_head_ok(x, lins, "relu"))
                            assert yes == B.head_ok("bf16" if dtype == torch.bfloat16 else "f32", 2, True, N, K0, addr, widths, ks, [rg] * len(widths))
                            assert not ops.mlp_head_ok(x, lins, "ssp")
                            if yes:
                                n_yes += 1
                                for direction in ("fwd", "bwd"):
                                    assert B.mlp_accepts(direction, N, K0, widths, x=addr) == B.OK, (N, K0, addr, widths)
    assert n_yes > 20


def test_allowed_is_within_its_limits():
    assert set(B.ALLOWED) == set(B.MLP_TENSORS) | set(B.GRU_TENSORS) | {"loss"}
    assert all(2.0 <= v <= 5.0 for v in B.ALLOWED.values()), B.ALLOWED
    a, b, c = torch.randn(30, 8), torch.randn(30, 8), torch.randn(30, 8).double()
    assert B.ratio(a, b, c) == B.row_ratio(a, b, c), "without a floor, ratio IS row_ratio"


INT_CASES = [n for n, c in B.MLP_CASES.items() if c["kind"] == "int"]


@pytest.mark.parametrize("name", INT_CASES)
def test_the_integer_cases_are_exact_in_any_order(name):
    k = B.mlp_case(name)
    i = k["inputs"]
    for t in [i["x"], i["gy"]] + i["b"]:
        assert set(t.unique().tolist()) <= {-1.0, 0.0, 1.0}
    for w in i["w"]:
        assert set(w.unique().tolist()) <= {-1.0, 0.0, 1.0}
        assert int((w != 0).sum(1).max()) <= 2 and int((w != 0).sum(0).max()) <= 2
    grow = [float(h.abs().max()) for h in k["model_h"]]
    assert all(g <= lim for g, lim in zip(grow, (3, 7, 15, 31))), grow
    assert all(torch.equal(a.double(), b) for a, b in zip(k["model_h"], k["ref_h"])), "the forward is exact"
    hs = k["model_h"][:-1]
    mod, ref = B.mlp_backward(i, hs), B.mlp_backward(i, hs, torch.float64, rounded=False)
    # dZ grows 1 -> 2 -> 4 -> 8 at the most; every partial sum of dW and db is an integer below 2^24
    dz = i["gy"].double()
    for l in range(i["NL"] - 1, -1, -1):
        a = (i["x"] if l == 0 else hs[l - 1]).double()
        assert float(dz.abs().max()) <= 2 ** (i["NL"] - 1 - l)
        assert float((dz.abs().t() @ a.abs()).max()) < 2 ** 24 and float(dz.abs().sum(0).max()) < 2 ** 24
        assert torch.equal(mod["dw"][l].double(), ref["dw"][l]) and torch.equal(mod["db"][l].double(), ref["db"][l])
        dz = (dz @ i["w"][l].double()) * ((hs[l - 1] > 0) if l else 1.0)
    assert torch.equal(mod["dx"].double(), ref["dx"]) and float(mod["dx"].abs().max()) <= 256


@pytest.mark.parametrize("name", list(B.MLP_CASES))
def test_mlp_model_is_sane_and_inside_the_derived_bounds(name):
    k = B.mlp_case(name)
    i, c = k["inputs"], k["spec"]
    for t in [i["x"]] + i["w"] + [b for b in i["b"] if b is not None] + ([] if i["f32io"] else [i["gy"]]):
        assert torch.equal(B.bfr(t), t), "exact in bf16"
    if i["f32io"]:
        assert not torch.equal(B.bfr(i["gy"]), i["gy"]), "the fp32 gradient is NOT exact in bf16: the kernel has to round it"
    # the reference is the textbook chain
    a = i["x"].double()
    for l in range(i["NL"]):
        a = torch.nn.functional.linear(a, i["w"][l].double(), None if i["b"][l] is None else i["b"][l].double())
        a = torch.relu(a) if l + 1 < i["NL"] else a
        assert float((a - k["ref_h"][l]).abs().max()) <= 1e-12 * (1 + float(a.abs().max()))
    # the backward reference against autograd in fp64
    hs64 = [h.detach() for h in k["ref_h"][:-1]]
    x = i["x"].double().requires_grad_(True)
    ws = [w.double().requires_grad_(True) for w in i["w"]]
    bs = [None if b is None else b.double().requires_grad_(True) for b in i["b"]]
    a = x
    for l in range(i["NL"]):
        a = torch.nn.functional.linear(a, ws[l], bs[l])
        a = torch.relu(a) if l + 1 < i["NL"] else a
    a.backward(i["gy"].double())
    ref = B.mlp_backward(i, hs64, torch.float64, rounded=False)
    scale = lambda t: 1e-11 * (1 + float(t.abs().max()))
    for l in range(i["NL"]):
        assert float((ref["dw"][l] - ws[l].grad).abs().max()) <= scale(ws[l].grad)
        assert (ref["db"][l] is None) == (bs[l] is None) and (bs[l] is None or float((ref["db"][l] - bs[l].grad).abs().max()) <= scale(bs[l].grad))
    assert (ref["dx"] is None) == (not c["dx"]) and (ref["dx"] is None or float((ref["dx"] - x.grad).abs().max()) <= scale(x.grad))
    if c["kind"] == "cancel":
        s = i["x"].double() @ i["w"][0].double().t()
        mag = i["x"].double().abs() @ i["w"][0].double().abs().t()
        share = float((s.abs() <= 2.0 ** -6 * mag).double().mean())
        assert share > 0.5 and 0.2 < float((s > 0).double().mean()) < 0.8, share
    if c["kind"] == "dead":
        pre = i["x"].double() @ i["w"][0].double().t() + i["b"][0].double()
        assert float(pre.max()) < 0 and all(float(i["b"][l].max()) < 0 for l in range(i["NL"] - 1))
        assert all(float(h.abs().max()) == 0.0 for h in k["model_h"][:-1])
    # the model against itself: inside every interval and every bound, no failure at all
    fails, rep = B.mlp_judge_fwd(i, k["model_h"])
    assert not fails and all(v in (0.0, pytest.approx(1.0)) for v in rep["ratios"].values()), (fails, rep)
    hs = k["model_h"][:-1]
    fails, repb = B.mlp_judge_bwd(i, hs, B.mlp_backward(i, hs))
    assert not fails and all(v <= 1.0 for v in repb["bound"].values()) and repb["agree"] in (None, 1.0), (fails, repb)
    print("%s: single-valued intervals %s   model bound fractions %s" % (name, ["%.3f" % v for v in rep["single"]], repb["bound"]))


@pytest.mark.parametrize("name", list(B.GRU_CASES))
def test_gru_model_is_sane(name):
    k = B.gru_case(name)
    i, c = k["inputs"], k["spec"]
    if i["bf16"]:
        assert all(torch.equal(B.bfr(i[q]), i[q]) for q in ("gi", "gh")) and (i["g_lp"] is None or torch.equal(B.bfr(i["g_lp"]), i["g_lp"]))
    # the reference against autograd of the textbook step in fp64 (torch's sigmoid / tanh, h' = (1 - z) n + z h)
    gi, gh, h = (i[q].double().requires_grad_(True) for q in ("gi", "gh", "h"))
    C = i["C"]
    r = torch.sigmoid(gi[:, :C] + gh[:, :C])
    z = torch.sigmoid(gi[:, C:2 * C] + gh[:, C:2 * C])
    n = torch.tanh(gi[:, 2 * C:] + r * gh[:, 2 * C:])
    hn = (1 - z) * n + z * h
    g = sum(t.double() for t in (i["g_h"], i["g_lp"]) if t is not None)
    hn.backward(g)
    ref = k["ref"]
    assert float((ref["h_out"] - hn.detach()).abs().max()) <= 1e-14
    for key, t in (("dgi", gi), ("dgh", gh), ("dh", h)):
        assert float((ref[key] - t.grad).abs().max()) <= 1e-13 * (1 + float(t.grad.abs().max())), key
    if c["kind"] == "saturated":
        assert float(i["gi"].abs().max()) > 11 and float((1 - n.detach() ** 2).min()) < 1e-8
    if c["kind"] == "zero_state":
        assert float(i["h"].abs().max()) == 0.0
    fails, rat = B.gru_judge(i, k["model"], k["model"], ref)
    # (saturated: the floor under dgi / dgh may lie above the model's own error)
    assert not fails and all(v in (0.0, pytest.approx(1.0)) or (c["kind"] == "saturated" and v < 1.0) for v in rat.values()), (fails, rat)


@pytest.mark.parametrize("name", list(B.LOSS_CASES))
def test_loss_model_is_sane_and_inside_the_derived_bound(name):
    k = B.loss_case(name)
    i = k["inputs"]
    fn = torch.nn.functional.l1_loss if i["kind"] == 0 else torch.nn.functional.mse_loss
    p = i["p"][:i["n"]].double().requires_grad_(True)
    want = fn(p, i["y"].double())
    want.backward()
    assert abs(float(k["ref"]["loss"]) - float(want.detach())) <= 1e-14 * (1 + float(want.detach()))
    assert float((k["model"]["grad"][:i["n"]].double() - p.grad).abs().max()) <= 3 * B.U * float(p.grad.abs().max()) + 1e-30
    if i["data"] == "ties":
        assert 0.3 < float((i["p"][:i["n"]] == i["y"]).float().mean()) < 0.4
        assert i["kind"] == 1 or float(k["model"]["grad"][:i["n"]][i["p"][:i["n"]] == i["y"]].abs().max()) == 0.0
    if i["data"] == "int":
        assert float(k["model"]["terms"].double().sum()) < 2 ** 24
    fails, rep = B.loss_judge(i, k["model"], k["model"], k["ref"])
    assert not fails and rep["bound"] <= 1.0, (fails, rep)


APPLICABLE = []
for _m, (_fam, _ok) in B.MUTATIONS.items():
    _cases = B.MLP_CASES if _fam.startswith("mlp") else (B.GRU_CASES if _fam == "gru" else B.LOSS_CASES)
    APPLICABLE += [(n, _m) for n, c in _cases.items() if _ok(c)]
# (the two largest integer cases take seconds each on the CPU: one mutation of each kind is enough there)
APPLICABLE = [(n, m) for n, m in APPLICABLE if not (n in ("trip2_fwd_int", "trip2_bwd_int_det") and m != "trip2_rows_missing")
              and not (n.startswith("trip2_") and B.MUTATIONS[m][0] == "gru" and m not in ("tail_columns_dropped", "out_lp_rounded_twice"))]


@pytest.mark.parametrize("name,mutation", APPLICABLE)
def test_every_mutation_breaks_the_budget(name, mutation):
    """A condition, not a measurement: on the inputs of every case it applies to, each mutation stands at least 2 x ALLOWED over
    the model in the tight measure, or leaves a derived interval or bound, or breaks an equality of the GPU test."""
    fails = B.mutated_fails(name, mutation)
    print("%s / %s: %s" % (name, mutation, fails[:3]))
    assert fails, (name, mutation)


def test_mutations_apply_where_they_can_show():
    assert set(B.MUTATIONS) == {"drop_kstep", "skip_last_bias", "relu_last", "mask_ge", "hidden_fp32", "dz_not_rounded", "gy_not_rounded",
                                "ragged_rows_missing", "trip2_rows_missing", "nan_rows_included", "w_untransposed", "db_wrong_layer",
                                "dirty_pad_columns", "gate_order_zrn", "n_gate_r_outside", "dgh_n_without_r", "dh_without_z", "g_lp_ignored",
                                "out_lp_rounded_twice", "tail_columns_dropped", "mean_over_n_total", "tie_gradient_plus", "tail_not_zeroed",
                                "waves_dropped"}
    count = {m: sum(1 for n, mm in APPLICABLE if mm == m) for m in B.MUTATIONS}
    assert all(v >= 1 for v in count.values()), count
    assert ("trip2_bwd_int", "trip2_rows_missing") in APPLICABLE and ("ref_batch_f32io", "gy_not_rounded") in APPLICABLE
    assert ("four_layers", "w_untransposed") in APPLICABLE and ("ragged_widths", "dirty_pad_columns") in APPLICABLE
