"""The error budget of tests/stream_budget.py, checked without a GPU: the mirrors of the two dispatches put every case on the route
it is named after and reach every instantiation of csrc/bn.hip and csrc/segment.hip, the reference is the textbook formula, the
rounding model stays inside every derived bound, and every mutation of it (a kernel bug in miniature) breaks what
test_gpu_stream_budget.py enforces."""
import os
import re

import pytest
import torch

import stream_budget as B

CSRC = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "matdeeplearn_amd", "csrc")

# derived by hand from csrc/bn.hip: (W, CG, threads, rows per block, reduce grid, apply grid)
_B64, _F64, _B100 = (8, 8, 256, 32, 2, 3), (4, 16, 256, 16, 3, 5), (4, 25, 250, 10, 5, 9)
BN_ROUTES = {
    "b8_n1031": (8, 1, 256, 256, 1, 2), "b64_n257": _B64, "b136_n130": (8, 17, 255, 15, 2, 3), "b256_n70": (8, 32, 256, 8, 2, 3),
    "b100_n333": _B100, "b4_n5": (4, 1, 256, 256, 1, 1), "f4_n3": (4, 1, 256, 256, 1, 1), "f64_n257": _F64,
    "f252_n130": (4, 63, 252, 4, 5, 8), "f256_n4097": (4, 64, 256, 4, 129, 257), "b64_n1": (8, 8, 256, 32, 1, 1), "b64_n2": (8, 8, 256, 32, 1, 1),
    "f256_n32773_cap": (4, 64, 256, 4, 1024, 768), "b64_n262147_cap": (8, 8, 256, 32, 1024, 768),
    "far_f32": (4, 16, 256, 16, 32, 64), "far_bf16": (8, 8, 256, 32, 16, 32), "outlier0_f32": (4, 16, 256, 16, 32, 64),
    "outlier0_bf16": (8, 8, 256, 32, 16, 32), "relu_b64": _B64, "relu_b100": _B100, "shiftrow_b64": (8, 8, 256, 32, 2, 3),
    "shiftrow_f100": (4, 25, 250, 10, 2, 4), "no_affine_b64": _B64, "no_running_f64": _F64, "det_b64_n1031": (8, 8, 256, 32, 1, 9),
    "det_f100_n1031": (4, 25, 250, 10, 1, 26),
}
for _n in B.NDEV_ROWS:
    BN_ROUTES["ndev%d_b64" % _n], BN_ROUTES["ndev%d_f100" % _n] = (8, 8, 256, 32, 2, 3), (4, 25, 250, 10, 4, 8)

# derived by hand from csrc/segment.hip, per shape: forward route (sum / mean), backward route
SEG_ROUTES = {
    "small_b64": (("small", 8, 8), ("bwd_vec", 8, 8, False)), "small_b100": (("small", 4, 25), ("bwd_vec", 4, 25, False)),
    "small_f48": (("small", 4, 12), ("bwd_vec", 4, 12, False)), "small_f1024": (("small", 4, 256), ("bwd_vec", 4, 256, False)),
    "vec4_b64": (("vec", 8, 8, 4), ("bwd_vec", 8, 8, False)), "vec4_f64": (("vec", 4, 16, 4), ("bwd_vec", 4, 16, False)),
    "vec1_b48": (("vec", 8, 6, 1), ("bwd_vec", 8, 6, False)), "vec1_b100": (("vec", 4, 25, 1), ("bwd_vec", 4, 25, False)),
    "vec1_f48": (("vec", 4, 12, 1), ("bwd_vec", 4, 12, False)), "below_b64": (("small", 8, 8), ("bwd_vec", 8, 8, False)),
    "trip2_b64": (("vec", 8, 8, 4), ("bwd_vec", 8, 8, False)), "bwdtrip2_b64": (("vec", 8, 8, 4), ("bwd_vec", 8, 8, False)),
    "scalar_b50": (("scalar",), ("bwd_scalar",)), "scalar_f50": (("scalar",), ("bwd_scalar",)),
    "scalar_f64_off4": (("scalar",), ("bwd_vec", 4, 16, False)),
    "max_b50": (("scalar",), ("bwd_max",)), "max_f50": (("scalar",), ("bwd_max",)), "max_b64": (("scalar",), ("bwd_max",)),
    "max_f64": (("scalar",), ("bwd_max",)),
}

# every hipLaunchKernelGGL instantiation of the two files
_SM = ("sum", "mean")
BN_INSTANCES = ({("bn_reduce_kernel", t, m, w) for (t, w) in (("bf16", 8), ("bf16", 4), ("f32", 4)) for m in (0, 1)}
                | {("bn_apply_kernel", t, w) for (t, w) in (("bf16", 8), ("bf16", 4), ("f32", 4))}
                | {("bn_bwd_apply_kernel", "bf16", w, mask) for w in (8, 4) for mask in (False, True)} | {("bn_bwd_apply_kernel", "f32", 4, False)})
SEG_INSTANCES = ({(k, t, r, w) for k in ("seg_fwd_small_kernel", "seg_fwd_vec_kernel", "seg_bwd_vec_kernel")
                  for (t, w) in (("bf16", 8), ("bf16", 4), ("f32", 4)) for r in _SM}
                 | {("seg_fwd_kernel", t, r) for t in ("bf16", "f32") for r in _SM + ("max",)}
                 | {("seg_bwd_kernel", t, r) for t in ("bf16", "f32") for r in _SM}
                 | {("seg_bwd_max_kernel", t) for t in ("bf16", "f32")} | {("csr_rowptr_kernel",)})


def test_every_case_is_pinned_to_its_route():
    assert set(B.BN_CASES) == set(BN_ROUTES)
    for name, c in B.BN_CASES.items():
        assert B.bn_case_route(c) == BN_ROUTES[name], (name, B.bn_case_route(c))
    assert {c["shape"] for c in B.SEG_CASES.values()} == set(SEG_ROUTES)
    for name, c in B.SEG_CASES.items():
        r = B.seg_case_routes(c)
        assert (r["fwd"], r["bwd"]) == SEG_ROUTES[c["shape"]], (name, r)
        if c["add"]:
            assert r["bwd_add"] == r["bwd"][:3] + (True,), (name, r)


def test_every_instantiation_is_reached():
    """a condition, not a measurement: the instantiations are listed here and ticked off by case; the number of launch sites in
    the two files is pinned, so a new one cannot arrive without a case"""
    bn = set().union(*(B.bn_instances(c) for c in B.BN_CASES.values()))
    assert bn == BN_INSTANCES, (BN_INSTANCES - bn, bn - BN_INSTANCES)
    seg = set().union(*(B.seg_instances(c) for c in B.SEG_CASES.values()))
    assert seg == SEG_INSTANCES, (SEG_INSTANCES - seg, seg - SEG_INSTANCES)
    sites = {f: len(re.findall(r"hipLaunchKernelGGL\(", open(os.path.join(CSRC, f)).read())) for f in ("bn.hip", "segment.hip")}
    # bn.hip: one site per instantiation.  segment.hip: 4 small + 4 vec + 3 scalar + 4 bwd_vec + 2 bwd + 1 bwd_max + 1 rowptr sites, the
    # templates on the element type instantiated for both (the W = 4 sites for bf16 alone)
    assert sites == {"bn.hip": len(BN_INSTANCES), "segment.hip": 19}, sites
    assert len(SEG_INSTANCES) == 3 * 6 + 6 + 4 + 2 + 1
    # every forward shape runs with and without perm, for sum and mean; the large-N and the threshold shapes are what they claim
    for s in B.SEG_SHAPES:
        assert {(c["reduce"], c["perm"]) for c in B.SEG_CASES.values() if c["shape"] == s} == {(r, p) for r in _SM for p in (False, True)}
    sh = B.SEG_SHAPES
    assert sh["vec4_b64"]["N"] * 8 == 65536 and sh["below_b64"]["N"] == sh["vec4_b64"]["N"] - 1 and sh["vec4_f64"]["N"] * 16 == 65536
    assert all(65536 <= sh[k]["N"] * cg < 65536 + cg for k, cg in (("vec1_b48", 6), ("vec1_b100", 25), ("vec1_f48", 12)))
    assert sh["trip2_b64"]["N"] * 8 * 4 > 4096 * 256 and B.seg_grid(sh["trip2_b64"]["N"] * 8 * 4) == 4096
    assert int(B.seg_sizes(sh["bwdtrip2_b64"]).sum()) == 131200 and 131200 * 8 > 4096 * 256
    assert B.seg_sizes(sh["small_f1024"]).tolist() == [0, 1000, 7]
    mixed = B.seg_sizes(sh["vec4_b64"])
    assert int(mixed[0]) == 0 and int(mixed[-1]) == 0 and int(mixed.max()) == 1000 and set(range(10)) <= set(mixed.tolist())
    # BatchNorm: the grid caps make second trips (reduce: 4 rows in flight per lane and trip; apply: 4, backward apply: 2 per thread)
    W, CG, thr, rows, gr, ga = BN_ROUTES["f256_n32773_cap"]
    assert (gr, ga) == (1024, 768) and B.cdiv(32773, 4 * gr * rows) == 3 and 32773 % (4 * gr * rows) < gr * rows
    assert B.cdiv(32773 * CG, 4 * ga * thr) == 3 and B.cdiv(32773 * CG, 2 * ga * thr) == 6
    assert B.cdiv(B.BN_CASES["b64_n262147_cap"]["N"], 32 * 8) == 1025
    assert {BN_ROUTES[k][2] for k in ("b100_n333", "b136_n130", "f252_n130")} == {250, 255, 252}


def test_the_mirrors_at_the_edges_of_every_branch():
    assert B.bn_route(8, "bf16", 100)[:2] == (8, 1) and B.bn_route(12, "bf16", 100)[:2] == (4, 3) and B.bn_route(8, "f32", 100)[:2] == (4, 2)
    assert B.bn_route(148, "bf16", 100)[:4] == (4, 37, 222, 6) and B.bn_route(256, "f32", 100)[:4] == (4, 64, 256, 4)
    assert [B.bn_route(64, "bf16", n)[4] for n in (1, 256, 257, 1024 * 256, 1024 * 256 + 1)] == [1, 1, 2, 1024, 1024]
    assert [B.bn_route(64, "bf16", n)[5] for n in (1, 128, 129, 768 * 128, 768 * 128 + 1)] == [1, 1, 2, 768, 768]
    assert B.bn_route(64, "bf16", 10 ** 6, det=True)[4:] == (1, 768)
    for bad in ((2, "bf16"), (260, "f32"), (66, "f32"), (150, "bf16")):      # (C = 150 is no multiple of 4: bn_check refuses it)
        with pytest.raises(AssertionError):
            B.bn_route(bad[0], bad[1], 10)
    fwd = lambda red, dt, N, C, mods=(0, 0): B.seg_route("fwd", red, dt, N, 10 * N, C, mods)
    assert fwd("sum", "bf16", 8191, 64) == ("small", 8, 8) and fwd("sum", "bf16", 8192, 64) == ("vec", 8, 8, 4)
    assert fwd("mean", "bf16", 65536, 8) == ("vec", 8, 1, 4) and fwd("mean", "bf16", 65535, 8) == ("small", 8, 1)
    assert fwd("sum", "f32", 3, 1024) == ("small", 4, 256) and fwd("sum", "f32", 3, 1028) == ("vec", 4, 257, 1)
    assert fwd("sum", "f32", 70000, 64) == ("vec", 4, 16, 4) and fwd("sum", "f32", 70000, 128) == ("vec", 4, 32, 1)
    assert fwd("sum", "bf16", 70000, 96) == ("vec", 8, 12, 1) and fwd("sum", "bf16", 70000, 100) == ("vec", 4, 25, 1)
    # vector width from the bases: 16 bytes, else 8 bytes of bf16, else scalar
    assert fwd("sum", "bf16", 37, 64, (8, 0)) == ("small", 4, 16) and fwd("sum", "bf16", 37, 64, (0, 4)) == ("scalar",)
    assert fwd("sum", "f32", 37, 64, (4, 0)) == ("scalar",) and fwd("sum", "f32", 37, 64, (8, 0)) == ("scalar",) and fwd("max", "f32", 37, 64) == ("scalar",)
    assert fwd("sum", "bf16", 0, 64) == ("none",)
    bwd = lambda kind, red, dt, C, mods: B.seg_route(kind, red, dt, 37, 500, C, mods)
    assert bwd("bwd", "mean", "bf16", 64, (0, 0)) == ("bwd_vec", 8, 8, False) and bwd("bwd", "mean", "bf16", 64, (8, 0)) == ("bwd_vec", 4, 16, False)
    assert bwd("bwd_add", "sum", "bf16", 64, (0, 0, 8)) == ("bwd_vec", 4, 16, True) and bwd("bwd_add", "sum", "bf16", 64, (0, 0, 4)) == ("unsupp",)
    assert bwd("bwd_add", "sum", "f32", 50, (0, 0, 0)) == ("unsupp",) and bwd("bwd", "max", "f32", 64, (0, 0)) == ("bwd_max",)
    assert bwd("bwd", "sum", "bf16", 50, (0, 0)) == ("bwd_scalar",)


def test_allowed_is_within_its_limits():
    assert set(B.ALLOWED) == set(B.BN_TENSORS) | set(B.SEG_TENSORS)
    assert all(2.0 <= v <= 5.0 for v in B.ALLOWED.values()), B.ALLOWED


@pytest.mark.parametrize("name", list(B.BN_CASES))
def test_batchnorm_model_is_sane_and_inside_the_derived_bounds(name):
    c = B.bn_case(name)
    i, s = c["inputs"], c["spec"]
    ref, mod = c["ref"], c["model"]
    N = i["N"]
    if i["bf16"]:
        assert all(torch.equal(B.bfr(i[k]), i[k]) for k in ("x", "dy")), "exact in bf16"
    # the reference is the textbook formula
    x, dy = i["x"].double(), i["dy"].double()
    g = torch.ones(i["C"], dtype=torch.float64) if i["gamma"] is None else i["gamma"].double()
    b = torch.zeros(i["C"], dtype=torch.float64) if i["beta"] is None else i["beta"].double()
    mean, var = x.mean(0), x.var(0, unbiased=False)
    istd = (var + B.EPS).rsqrt()
    xhat = (x - mean) * istd
    ind = dict(mean=mean, invstd=istd, y=xhat * g + b, dbeta=dy.sum(0), dgamma=(dy * xhat).sum(0))
    ind["dx"] = g * istd * (dy - ind["dbeta"] / N - xhat * ind["dgamma"] / N)
    if s["relu"]:
        ind["dx"] = ind["dx"] * (x > 0)
        assert 0.3 < float((i["x"] == 0).float().mean()) < 0.7, "x is a ReLU output"
    if i["rm0"] is not None:
        ind["rm"] = (1 - B.MOM) * i["rm0"].double() + B.MOM * mean
        ind["rv"] = (1 - B.MOM) * i["rv0"].double() + B.MOM * (x.var(0, unbiased=True) if N > 1 else var)
    assert set(ind) == set(ref) - {"s0", "s1"}
    for k, v in ind.items():
        # (the fp64 reference forms the variance about row 0 too: 1e-9 leaves room for 2^-53 (1 + delta^2 / sigma^2), delta = 64 sigma)
        tol = 1e-9 * (float(v.abs().max()) + 1e-30) + (1e-9 if k in ("dx", "dgamma") else 0.0)
        assert float((ref[k] - v).abs().max()) <= tol, (name, k, float((ref[k] - v).abs().max()))
    if s["kind"] == "outlier0":
        col = x[:, B.HARD_COLUMN]
        assert float((col[0] - col.mean()).abs() / col[1:].std()) > 60.0
    if s["kind"] == "far":
        assert 39.0 < float(mean[B.HARD_COLUMN]) < 41.0 and float(var[B.HARD_COLUMN]) < 0.05
    # the model against itself, and inside every derived bound
    r = B.bn_ratios(mod, mod, ref)
    assert all(v in (0.0, pytest.approx(1.0)) or (ref[k].dim() == 1 and v < 1.0) for k, v in r.items()), r   # (vec_ratio: floored)
    f, exact = B.bn_bound_fraction(mod, i)
    print("%s: model bound fractions %s" % (name, f))
    assert all(v <= 1.0 for v in f.values()), (name, f)
    if s["kind"] == "ints":
        assert torch.equal(mod["s0"].double(), exact["s0"]) and torch.equal(mod["s1"].double(), exact["s1"])
        assert float(exact["s1"].max()) < 2 ** 24 and torch.equal(mod["dbeta"].double(), ref["dbeta"])
    if N == 1:
        assert float(mod["invstd"].min()) == float(mod["invstd"].max()) and float(ref["dx"].abs().max()) == 0.0


@pytest.mark.parametrize("name", list(B.SEG_CASES))
def test_segment_model_is_sane_and_inside_the_derived_bound(name):
    c = B.seg_case(name)
    i, s = c["inputs"], c["spec"]
    ref, mod = c["ref"], c["model"]
    N, E, C = i["N"], i["E"], i["C"]
    if i["bf16"]:
        assert all(torch.equal(B.bfr(i[k]), i[k]) for k in ("src", "go")), "exact in bf16"
    # the reference is scatter over the segment index of every source row
    cnt = i["rowptr"][1:] - i["rowptr"][:-1]
    rows = torch.arange(E) if i["perm"] is None else i["perm"]
    seg_of_row = torch.empty(E, dtype=torch.int64)
    seg_of_row[rows] = torch.repeat_interleave(torch.arange(N), cnt)
    src, go = i["src"].double(), i["go"].double()
    if i["reduce"] == "max":
        ind = torch.stack([src[seg_of_row == n].max(0).values if int(cnt[n]) else torch.zeros(C, dtype=torch.float64) for n in range(N)])
        assert torch.equal(ref["out"], ind) and torch.equal(mod["out"].double(), ind)
        am = mod["argmax"].long()
        assert bool((am[cnt == 0] == -1).all()) and bool((am[cnt > 0] >= 0).all()) and torch.equal(ref["argmax"], mod["argmax"])
        n_i, c_i = (am >= 0).nonzero(as_tuple=True)
        assert torch.equal(src[am[n_i, c_i], c_i], ind[n_i, c_i]) and bool((seg_of_row[am[n_i, c_i]] == n_i).all())
        # first maximum: no earlier slot of the segment holds the same value
        slot = torch.empty(E, dtype=torch.int64)
        slot[rows] = torch.arange(E)
        ties = 0
        for n, ch in zip(n_i[::7].tolist(), c_i[::7].tolist()):
            seg_vals = src[rows[i["rowptr"][n]:slot[am[n, ch]]], ch]
            assert bool((seg_vals < ind[n, ch]).all())
            ties += int((src[rows[i["rowptr"][n]:i["rowptr"][n + 1]], ch] == ind[n, ch]).sum() > 1)
        assert ties > 10, "the inputs hold ties"
        assert abs(float(mod["gsrc"].double().sum()) - float(go[cnt > 0].sum())) < 1e-9 and int((mod["gsrc"] != 0).sum()) <= N * C
        return
    ind = torch.zeros(N, C, dtype=torch.float64).index_add_(0, seg_of_row, src)
    div = cnt.clamp(min=1).double().unsqueeze(1) if i["reduce"] == "mean" else 1.0
    assert float((ref["out"] - ind / div).abs().max()) <= 1e-12 * float(ind.abs().max() + 1)
    assert float((ref["gsrc"] - (go / div)[seg_of_row]).abs().max()) <= 1e-12
    if i["addend"] is not None:
        assert float((ref["gsrc_add"] - ((go / div)[seg_of_row] + i["addend"].double())).abs().max()) <= 1e-12
    assert bool((ref["out"][cnt == 0] == 0).all()) and int((cnt == 0).sum()) >= (2 if s["sizes"] == "mixed" and N > 3 else 0)
    r = B.seg_ratios(mod, mod, ref)
    assert all(v in (0.0, pytest.approx(1.0)) for v in r.values()), r
    f = B.seg_bound_fraction(mod["out"], i)
    print("%s: model bound fraction %.3g" % (name, f))
    assert f <= 1.0
    if s["ints"]:
        assert all(torch.equal(mod[k].double(), ref[k]) for k in mod), "integer inputs: exact"


def _breaks(mut, c, tensors):
    """why a mutated model fails test_gpu_stream_budget.py: (reason, figure) or None"""
    for k, v in mut.items():
        if v.is_floating_point() and not bool(torch.isfinite(v).all()):
            return ("not finite", k)
    i = c["inputs"]
    if i.get("relu") and not bool((mut["dx"][i["x"] <= 0] == 0).all()):
        return ("dx not zero behind the ReLU", "dx")
    r = B.bn_ratios(mut, c["model"], c["ref"]) if "y" in mut else B.seg_ratios(mut, c["model"], c["ref"])
    own = [k for k in tensors if k in r]
    k = max(own, key=lambda k: r[k] / B.ALLOWED[k])
    return ("%s at %.3g x (allowed %.1f)" % (k, r[k], B.ALLOWED[k]), k) if r[k] >= 2.0 * B.ALLOWED[k] else None


APPLICABLE = [(n, m) for n in B.BN_CASES for m, (fam, ok, _) in B.MUTATIONS.items() if fam == "bn" and ok(B.BN_CASES[n])] + \
             [(n, m) for n in B.SEG_CASES for m, (fam, ok, _) in B.MUTATIONS.items() if fam == "seg" and ok(B.SEG_CASES[n])]


@pytest.mark.parametrize("name,mutation", APPLICABLE)
def test_every_mutation_breaks_the_budget(name, mutation):
    """A condition, not a measurement: on the inputs of every case it applies to, each mutation stands at least 2 x ALLOWED over
    the model in one of the tensors it models, or breaks an equality or a finiteness assertion of the GPU test."""
    fam, _, tensors = B.MUTATIONS[mutation]
    c = B.bn_case(name) if fam == "bn" else B.seg_case(name)
    mut = (B.bn_compute if fam == "bn" else B.seg_compute)(c["inputs"], mutation=mutation)
    why = _breaks(mut, c, tensors)
    print("%s / %s: %s" % (name, mutation, why))
    assert why is not None, (name, mutation)


def test_mutations_apply_where_they_can_show():
    assert set(B.MUTATIONS) == {"drop_replica", "shift_row1", "pad_row_counted", "rv_biased", "relu_mask_lt", "no_xhat_term",
                                "mean_noclamp", "lane_dropped", "tail_twice", "perm_ignored", "addend_omitted"}
    count = {m: sum(1 for n, mm in APPLICABLE if mm == m) for m in B.MUTATIONS}
    assert all(v >= 2 for v in count.values()), count
    # the stored shift row and the sixteen copies are pinned by the apply-alone cases
    assert ("shiftrow_b64", "drop_replica") in APPLICABLE and ("shiftrow_f100", "shift_row1") in APPLICABLE
    reps = B.bn_case("shiftrow_b64")["inputs"]["replicas"]
    assert reps.shape == (B.R, 2, 64) and len({tuple(t.flatten().tolist()) for t in reps}) == B.R, "sixteen different copies"
