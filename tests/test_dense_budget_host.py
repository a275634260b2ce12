"""The error budget of tests/dense_budget.py, checked without a GPU: the mirrors of the two launchers' dispatch put every case on
the route it is named after and reach every instantiation, the rounding model is the reference when its roundings are switched
off, every mutation of it (a kernel bug in miniature) breaks the budget that test_gpu_dense_budget.py enforces, and the kernel's
summation order, emulated on the CPU, stays inside both measures — the inputs leave the reference side room."""
import pytest
import torch

import dense_budget as B

S, F = "stream", "fallback"
ROUTES = {   # derived by hand from csrc/gemm_tn.hip and csrc/dense_bwd.hip: (kind, mt, nt, NW, grid, part) / (fallback, mt, ntw, grid)
    "t11_k30": (S, 1, 1, 4, 1, False), "t12_k32": (S, 1, 2, 4, 1, False), "t14_k94": (S, 1, 4, 4, 1, False),
    "t15_k128": (S, 1, 5, 8, 1, False), "t21": (S, 2, 1, 4, 2, False), "t22": (S, 2, 2, 4, 2, False),
    "t24_k96": (S, 2, 4, 4, 4, False), "t25_k158": (S, 2, 5, 8, 4, False), "t41_m66": (S, 4, 1, 4, 1, False),
    "t42": (S, 4, 2, 4, 2, False), "t44": (S, 4, 4, 4, 2, False), "t45_k160": (S, 4, 5, 8, 1, False),
    "t51": (S, 5, 1, 8, 1, False), "t52": (S, 5, 2, 8, 1, False), "t54": (S, 5, 4, 8, 4, False), "t55": (S, 5, 5, 8, 2, False),
    "det200": (S, 2, 2, 4, 1, False), "prefetch": (S, 2, 2, 4, 256, False), "cap512": (S, 1, 1, 4, 512, False),
    "part_off": (S, 2, 2, 4, 31, False), "part_on": (S, 2, 2, 4, 32, True), "part_on_bumped": (S, 4, 4, 4, 33, True),
    "scratch_misaligned": (S, 2, 2, 4, 32, False), "prefill": (S, 2, 2, 4, 4, False), "strided": (S, 1, 1, 4, 2, False),
    "strided_wide": (S, 5, 4, 8, 4, False),
    "fb11_base2": (F, 1, 1, 2), "fb21_odd_m": (F, 2, 1, 2), "fb31_odd_k": (F, 3, 1, 2), "fb41_odd_lda": (F, 4, 1, 2),
    "fb12_k200": (F, 1, 2, 2), "fb22_k200": (F, 2, 2, 1), "fb32_k256": (F, 3, 2, 2), "fb42_k256": (F, 4, 2, 3),
    "fb51_m130_odd_lda": (F, 5, 1, 2),
    "d22": ("dx", 2, 2, 8, 1, False), "d24_k66": ("dx", 2, 4, 4, 1, False), "d25_k158": ("dx", 2, 5, 8, 1, False),
    "d42_m66": ("dx", 4, 2, 4, 1, False), "d44_k94": ("dx", 4, 4, 4, 2, False), "d44_nodb_k66": ("dx", 4, 4, 8, 2, False),
    "d45_k160": ("dx", 4, 5, 8, 2, False), "d52_m160": ("dx", 5, 2, 8, 4, False), "d54": ("dx", 5, 4, 8, 2, False),
    "d55": ("dx", 5, 5, 8, 4, False), "d_strided": ("dx", 4, 4, 4, 2, False), "d_strided_relu": ("dx", 2, 2, 4, 1, False),
    "d_det200": ("dx", 2, 2, 4, 1, False), "d_part_off": ("dx", 2, 2, 8, 31, False), "d_part_on": ("dx", 2, 2, 4, 32, True),
    "d_prefetch": ("dx", 2, 2, 4, 256, False), "d_prefill": ("dx", 2, 2, 8, 4, False),
}


def test_every_case_is_pinned_to_its_route():
    assert list(B.CASES) == list(ROUTES)
    for name, c in B.CASES.items():
        assert B.case_route(c) == ROUTES[name], (name, B.case_route(c))


def test_the_mirrors_at_the_edges_of_every_branch():
    tn = lambda M, K, cs=False, act=0, N=200, **kw: B.tn_route(M, K, cs, act, kw.pop("lda", M), kw.pop("ldb", K), kw.pop("a4", 0),
                                                              kw.pop("b4", 0), N, **kw)
    # tiles: 32 -> 1, 34 -> 2, 64 -> 2, 66 -> 3 -> 4, 96 -> 4, 128 -> 4, 130 -> 5
    assert [tn(M, 30)[1] for M in (2, 32, 34, 64, 66, 96, 98, 128, 130, 160)] == [1, 1, 2, 2, 4, 4, 4, 4, 5, 5]
    # the ones column: K = 30 stays in its tile, K = 32 opens one, 94 and 96 both land on 4, 128 opens the fifth, 160 has no sixth
    assert [tn(30, K, True)[2] for K in (30, 32, 62, 64, 94, 96, 126, 128, 158)] == [1, 2, 2, 4, 4, 4, 4, 5, 5]
    assert tn(30, 160, True) == ("unsupp", "colsum") and tn(30, 160)[:4] == (S, 1, 5, 8)
    assert tn(30, 162)[:3] == (F, 1, 2) and tn(30, 128)[:3] == (S, 1, 4) and tn(30, 256)[:3] == (F, 1, 2)
    # each reason for the fallback; an activation staging there is refused
    for kw in (dict(lda=31), dict(ldb=31), dict(a4=2), dict(b4=2)):
        assert tn(30, 30, **kw)[0] == F and tn(30, 30, act=1, **kw) == ("unsupp", "act") and tn(30, 30, True, **kw) == ("unsupp", "colsum")
    assert tn(31, 30)[0] == F and tn(30, 31)[0] == F
    # grid: one workgroup per tile up to 256; 512 from 2^20 rows unless 25 tiles; one when deterministic
    assert [tn(34, 34, N=n)[4] for n in (1, 64, 65, 16384, 16385, (1 << 20) - 1, 1 << 20)] == [1, 1, 2, 256, 256, 256, 512]
    assert tn(160, 158, True, N=1 << 20)[4] == 256 and tn(34, 34, N=1 << 20, det=True)[4] == 1
    assert [tn(33, 34, N=n)[3] for n in (128, 129, 65536, 65537)] == [1, 2, 512, 512] and tn(33, 34, det=True)[3] == 1
    # part: scratch, 16-byte aligned, not deterministic, at least 32 workgroups
    assert [tn(34, 34, N=n, scratch_mod16=0)[5] for n in (1984, 1985)] == [False, True]
    assert not tn(34, 34, N=1985, scratch_mod16=4)[5] and not tn(34, 34, N=1985)[5] and not tn(34, 34, N=1985, scratch_mod16=0, det=True)[5]
    # the one-pass backward: NW = 8 without an activation staging and on every 5-tile side
    assert B.dense_route(34, 66, False, 0, 100)[:4] == ("dx", 2, 4, 8) and B.dense_route(34, 64, False, 1, 100)[:4] == ("dx", 2, 2, 4)
    assert B.dense_route(34, 64, True, 1, 100)[:4] == ("dx", 2, 4, 4) and B.dense_route(34, 128, True, 2, 100)[:4] == ("dx", 2, 5, 8)
    assert B.dense_route(130, 34, True, 1, 100)[:4] == ("dx", 5, 2, 8) and B.dense_route(128, 128, False, 2, 100)[:4] == ("dx", 4, 4, 4)
    assert [B.dense_route(34, 34, True, 0, n, 0)[4:] for n in (1984, 1985)] == [(31, False), (32, True)]
    with pytest.raises(AssertionError):
        B.dense_route(34, 160, True, 0, 100)


def test_every_instantiation_is_reached():
    tn = {n: (B.case_route(c), c) for n, c in B.TN_CASES.items()}
    stream = {(r[1], r[2], c["act"], r[3]) for r, c in tn.values() if r[0] == S}
    assert {k[:2] for k in stream} == {(a, b) for a in (1, 2, 4, 5) for b in (1, 2, 4, 5)}
    assert {(k[2], k[3]) for k in stream} == {(a, nw) for a in (0, 1, 2) for nw in (4, 8)}
    # (5 row tiles: the <4, 1> and <1, 1> launches of one call)
    assert {r[1:3] for r, c in tn.values() if r[0] == F} == {(a, b) for a in (1, 2, 3, 4) for b in (1, 2)} | {(5, 1)}
    dn = {n: (B.case_route(c), c) for n, c in B.DENSE_CASES.items()}
    assert {r[1:3] for r, c in dn.values()} == {(a, b) for a in (2, 4, 5) for b in (2, 4, 5)}
    assert {(c["act"], r[3]) for r, c in dn.values()} == {(0, 8), (1, 4), (1, 8), (2, 4), (2, 8)}
    assert {c["xout"] for r, c in dn.values()} == {0, 1, 2} and {c["gm"] for r, c in dn.values()} == {False, True}
    assert {c["colsum"] for r, c in dn.values()} == {False, True}
    assert {c["N"] for c in B.TN_CASES.values()} >= {1, 33, 63, 64, 65, 96, 200, 16453, (1 << 20) + 1, 1984, 1985}
    assert {c["N"] for c in B.DENSE_CASES.values()} >= {1, 32, 33, 64, 65, 97, 200, 16453, 1984, 1985}
    assert {c["M"] for c in B.DENSE_CASES.values()} >= {34, 66, 96, 160} and {c["K"] for c in B.DENSE_CASES.values()} >= {34, 66, 94, 158, 160}
    # strided cases: every ld above its width, bases 4-byte but not 16-byte aligned
    for n in ("strided", "strided_wide", "d_strided", "d_strided_relu"):
        c = B.CASES[n]
        assert c["lda"] > c["M"] and c["ldb"] > c["K"] and c["ldy"] > c["M"] and all(c[k] % 2 == 0 and (2 * c[k]) % 16 for k in ("aoff", "boff", "yoff"))
    assert B.CASES["strided"]["lda"] - 30 == 6 and B.CASES["strided"]["ldb"] - 30 == 10 and B.CASES["strided"]["ldy"] - 30 == 2
    assert B.CASES["d_strided"]["lddx"] - 66 == 6
    # 16-dword rests: M = 130 stages 64 dwords per row with one load and the last 16 (one is a gutter) four rows at a time
    assert 16 * 5 // 64 == 1 and 16 * 5 % 64 == 16


def test_allowed_is_within_its_limits():
    assert set(B.ALLOWED) == set(B.TENSORS)
    assert all(2.0 <= v <= 5.0 for v in B.ALLOWED.values()), B.ALLOWED


@pytest.mark.parametrize("name", list(B.CASES))
def test_model_is_sane(name):
    c = B.case(name)
    i, s = c["inputs"], c["spec"]
    for k in ("g", "x", "y", "w", "g_pad", "x_pad", "a_gutter"):
        if i[k] is not None:
            assert torch.equal(B.bfr(i[k]), i[k]), (name, k)                   # exact in bf16
    if s["act"] == 1:
        assert float(i["y"].min()) == 0.0 and 0.3 < float((i["y"] == 0).float().mean()) < 0.7 or s["N"] == 1, "y is post-ReLU"
    if s["xout"] == 1:
        assert float(i["x"].min()) == 0.0
    # the model with its roundings switched off IS the reference; the reference is the formula of the layer's backward
    off = B.compute(i, torch.float64, rounded=False, colsum=s["colsum"])
    g, x = i["g"].double(), i["x"].double()
    d = B.dact(s["act"], i["y"], torch.float64) if s["act"] else torch.ones_like(g)
    ind = dict(dW=torch.einsum("nm,nm,nk->mk", g, d, x), db=(g * d).sum(0), gm=g * d)
    if i["C0"] is not None:
        ind["dW"], ind["db"] = ind["dW"] + i["C0"], ind["db"] + i["cs0"]
    if i["w"] is not None:
        ind["dX"] = torch.einsum("nm,mk->nk", g * d, i["w"].double()) * B.dact(s["xout"], i["x"], torch.float64)
    for k, v in c["ref"].items():
        scale = float(ind[k].abs().max()) + 1e-30
        assert float((off[k] - v).abs().max()) <= 1e-12 * scale and float((ind[k] - v).abs().max()) <= 1e-12 * scale, (name, k)
    assert set(c["ref"]) == {"dW", "gm"} | ({"db"} if s["colsum"] else set()) | ({"dX"} if s["kind"] == "dense" else set())
    r = B.ratios(c["model"], c["model"], c["ref"])
    assert all(v in (0.0, pytest.approx(1.0)) for v in r.values()), r
    if s["act"] != 2:
        assert torch.equal(c["model"]["gm"].double(), c["ref"]["gm"]), "g' is exact without a softplus factor"
    if s["ints"]:
        assert torch.equal(c["model"]["dW"].double(), c["ref"]["dW"]) and torch.equal(c["model"]["db"].double(), c["ref"]["db"])


APPLICABLE = [(n, m) for n in B.CASES for m in B.MUTATIONS if B.MUTATIONS[m][0](B.CASES[n])]


@pytest.mark.parametrize("name,mutation", APPLICABLE)
def test_every_mutation_breaks_the_budget(name, mutation):
    """A condition, not a measurement: on the inputs of every case it applies to, each mutation stands at least 2 x ALLOWED over the
    model in one of the tensors it models."""
    c = B.case(name)
    r = B.ratios(B.mutated(name, mutation), c["model"], c["ref"])
    own = [k for k in B.MUTATIONS[mutation][1] if k in r]
    witness = max(own, key=lambda k: r[k] / B.ALLOWED[k])
    print("%s / %s: %s at %.3gx (allowed %.1f)   all: %s" % (name, mutation, witness, r[witness], B.ALLOWED[witness], B.fmt(r)))
    assert r[witness] >= 2.0 * B.ALLOWED[witness], (name, mutation, r)
    for k in set(r) - set(B.MUTATIONS[mutation][1]):
        assert r[k] in (0.0, pytest.approx(1.0)), (mutation, k)


def test_mutations_apply_where_they_can_show():
    count = {m: sum(1 for n, mm in APPLICABLE if mm == m) for m in B.MUTATIONS}
    assert all(v >= 2 for v in count.values()), count
    assert count["drop_last_row"] == count["row_past_n"] == count["drop_tile"] == len(B.CASES)
    # staging a relu tile twice is no bug: the mask is idempotent
    c = B.case("t21")
    twice = B.model(c["inputs"], mutation="staged_twice")
    assert all(torch.equal(twice[k], c["model"][k]) for k in twice)


@pytest.mark.parametrize("name", list(B.CASES))
def test_model_and_emulated_kernel_order_stay_inside_both_measures(name):
    """The derived bound holds for the model, and for the kernel's summation order emulated in fp32 on the CPU, which also stays
    within ALLOWED of the model: a correct kernel has room on these inputs."""
    c = B.case(name)
    i, s = c["inputs"], c["spec"]
    emu = B.emulate(i, c["route"], s["colsum"])
    r = B.ratios(emu, c["model"], c["ref"])
    fm, fe = B.bound_fraction(c["model"], i, s["colsum"]), B.bound_fraction(emu, i, s["colsum"])
    print("%s: emulated order %s   bound fraction model %s   emulation %s" % (
        name, B.fmt(r), {k: "%.2g (%.2f u)" % v for k, v in fm.items()}, {k: "%.2g (%.2f u)" % v for k, v in fe.items()}))
    for k, v in r.items():
        assert v <= B.ALLOWED[k], (name, k, v)
    for f in (fm, fe):
        assert all(v[0] <= 1.0 for v in f.values()), (name, f)
    if s["ints"]:
        assert torch.equal(emu["dW"], c["model"]["dW"]) and all(v[1] == 0.0 for v in fe.values())


def test_the_old_tolerance_does_not_see_a_dropped_row():
    """Why this suite exists: close(dW, ref, 1e-4, 2e-5 sqrt(N)) of test_dense_bwd_matches_torch passes a dW that lacks one of
    16453 rows in nine elements of ten; the budget sees it thousands of times over."""
    c = B.case("d_prefetch")
    mut, ref = B.mutated("d_prefetch", "drop_last_row")["dW"].double(), c["ref"]["dW"]
    tol = 1e-4 * ref.abs() + 2e-5 * 16453 ** 0.5 * float(ref.abs().max())
    assert float(((mut - ref).abs() <= tol).double().mean()) > 0.9
    assert B.row_ratio(mut, c["model"]["dW"], ref) > 1000.0


@pytest.mark.parametrize("name", list(B.LAYER_CASES))
def test_layer_cases_are_what_their_names_say(name):
    M, K, act, need_dx, calls = B.LAYER_CASES[name]
    c = B.layer_case(name)
    for k, v in c["inputs"].items():
        assert torch.equal(B.bfr(v), v), (name, k)
    assert set(c["ref"]) == set(c["model"]) == {"dW", "db"} | ({"dX"} if need_dx else set())
    for k in c["ref"]:
        ref = c["ref"][k]
        assert c["model"][k].shape == ref.shape
        assert float((c["model"][k].double() - ref).abs().max()) <= 2e-2 * float(ref.abs().max()), (name, k)
    # the launches, from the arithmetic of ops._tn_plan restated
    if K > 256:
        kh = (K // 2 + 1) & ~1
        assert [(c_[3], c_[4], c_[6], c_[7]) for c_ in calls] == [(K, kh, kh <= 158, 0), (K, K - kh, False, (2 * kh) % 16)]
        assert kh == {258: 130, 300: 150, 320: 160}[K]
    elif M > 160:
        nch = -(-M // 150)
        mc = ((M + nch - 1) // nch + 1) & ~1
        spans = [(m0, min(m0 + mc, M)) for m0 in range(0, M, mc)]
        assert [(c_[1], c_[2], c_[3], c_[4], c_[7]) for c_ in calls] == [(K, K, M, b - a, (2 * a) % 16) for a, b in spans]
        assert all(c_[3] > c_[4] for c_ in calls), "strided slices of g"
    elif M % 2:
        assert calls == [("tn", M + 1, M + 1, K, K, 0, True, 0)]
    else:
        assert len(calls) == 1 and calls[0][0] == ("dense" if need_dx else "tn") and calls[0][5] == {"relu": 1, "ssp": 2}[act]
    # every launch lands on the streaming kernel
    for c_ in calls:
        if c_[0] == "tn":
            assert B.tn_route(c_[2], c_[4], c_[6], c_[5], c_[1], c_[3], 0, 0, B.LAYER_N)[0] == S
        else:
            assert B.dense_route(c_[2], c_[4], c_[6], c_[5], B.LAYER_N)[0] == "dx"


# ---------------------------------------------------------------------------------------------
# the admission windows of matdeeplearn_amd/ops.py against the mirrors of the launchers: what the host layer admits, the kernels take
# ---------------------------------------------------------------------------------------------
class _Rows:
    """what the shape predicates read of an operand: dense rows on a dword"""

    def __init__(self, rows, cols):
        self.shape = (rows, cols)

    def stride(self, d):
        return self.shape[1] if d == 0 else 1

    def data_ptr(self):
        return 0


def _inside(fn, *a):
    """the route, or None where the mirror's assertion of the launcher's domain fails"""
    try:
        return fn(*a)
    except AssertionError:
        return None


def test_one_pass_window_lies_inside_the_kernels():
    """Every shape the one-pass dense backward is given lies inside the window mdl_dense_bwd_ex asserts, with every activation
    code; the Linear -> ReLU -> BatchNorm node asks for nothing the one-pass window does not hold."""
    from matdeeplearn_amd import ops
    admitted, bad = 0, []
    for M in range(1, 200):
        for K in range(1, 300):
            for bias in (False, True):
                one_pass = ops._dense_bwd_shape_ok(M, K, bias)
                assert one_pass or not ops._dense_bwd_shape_ok(M, K, bias, wide=False)
                if one_pass:
                    admitted += 1
                    bad += [(M, K, bias, act) for act in (0, 1, 2) if _inside(B.dense_route, M, K, bias, act, B.LAYER_N) is None]
                for tables in range(5):
                    if ops._relu_bn_shape_ok(M, K, bias, tables):
                        assert ops._dense_bwd_shape_ok(M, K, bias, wide=False) and tables <= 3, (M, K, bias, tables)
    assert admitted == 8128 and not bad, (admitted, bad[:10])


def test_staged_activation_window_lands_on_the_streaming_kernel():
    """Where the fused forward and the column-sum / staged-activation window both admit a layer, the TN GEMM with the activation
    staged (and with the column sums, for a bias) is the streaming kernel: never refused, never the scalar-load fallback."""
    from matdeeplearn_amd import ops
    admitted, bad = 0, []
    for M in range(1, 200):
        for K in range(1, 300):
            for act, code in ((None, 0), ("relu", 1), ("ssp", 2)):
                if not (ops._fused_fwd_shape_ok(M, K, act) and ops._tn_colsum_shape_ok(M, K)):
                    continue
                for bias in (False, True):
                    admitted += 1
                    r = _inside(B.tn_route, M, K, bias, code, M, K, 0, 0, B.LAYER_N)
                    if r is None or r[0] != S:
                        bad.append((M, K, act, bias, r))
    assert admitted > 10000 and not bad, (admitted, bad[:10])


def test_every_launch_of_the_weight_gradient_plan_is_taken():
    """For every layer ops.linear admits (ops._linear_tn_ok: up to 600 outputs as transposed chunks, up to 512 inputs as column
    halves), every TN launch of ops._tn_plan — the plan ops._tn_dw_db itself walks — lies inside the domain mdl_gemm_tn_ex asserts,
    and a launch that carries column sums lands on the streaming kernel (the fallback refuses them)."""
    from matdeeplearn_amd import ops
    admitted, launches, bad = 0, 0, []
    for M in range(1, 602):
        for K in range(1, 514):
            if not ops._linear_tn_ok(_Rows(B.LAYER_N, K), _Rows(M, K)):
                continue
            admitted += 1
            Ma = M + M % 2                                                    # (an odd width is padded with a zero column)
            for bias in (False, True):
                for Mk, Kk, lda, ldb, colsum, lo, hi in ops._tn_plan(Ma, K, bias, Ma, K):
                    launches += 1
                    assert hi - lo == Kk, (M, K)                              # (the B operand is the column slice lo:hi)
                    r = _inside(B.tn_route, Mk, Kk, colsum, 0, lda, ldb, 0, (2 * lo) % 4, B.LAYER_N)
                    if r is None or r[0] not in ((S,) if colsum else (S, F)):
                        bad.append((M, K, bias, (Mk, Kk, lda, ldb, colsum, lo, hi), r))
    assert admitted > 40000 and launches > 2 * admitted and not bad, (admitted, launches, bad[:10])
