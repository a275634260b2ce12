"""The dense layers' forward on the device against the fp64 reference, within the measures of tests/linear_budget.py: per row within
ALLOWED times the error of the rounding model, every element inside the derived interval of admissible bf16 values, the BatchNorm
sums within their derived bounds of the kernel's own stored rows, integer cases bit-equal.
Op level: the five entry points of csrc/linear.hip through the C ABI on every route of their dispatch, the route computed from the
arguments and pointers actually passed.  The operands lie inside NaN-filled buffers (70 NaN rows behind x, y and g, NaN rows behind
w and the bias, one all-NaN row in every table that every index past N points at: a read outside poisons the result) and the
outputs are carved out of NaN-filled arenas (what must not be written stays NaN).  Every case is launched twice: the output has no
atomics and must be bit-equal.
Layer level: ops.linear_act / linear_gather_act / linear_relu_bn / matmul_wide on fp32 master weights, with the launches counted.
test_linear_budget_host.py shows that these checks can fail: every mutation of the model breaks the measure that owns it."""
import ctypes

import pytest
import torch

import linear_budget as B

pytestmark = pytest.mark.gpu
NAN = float("nan")
SENTINEL = 7.0                                   # what the totals rows of the sums buffer hold on entry


def dev():
    return torch.device("cuda:0")


class _Arena:
    """outputs of one dtype carved out of ONE NaN-filled allocation, GUARD bytes behind each; an output starts `off` elements
    behind a 16-byte boundary"""

    def __init__(self, specs, dtype, d):
        size = torch.empty(0, dtype=dtype).element_size()
        g, al = B.GUARD // size, 16 // size
        self.spans, pos = {}, g
        for name, rows, cols, off in specs:
            pos = (pos + al - 1) // al * al + off
            self.spans[name] = (pos, rows, cols)
            pos += rows * cols + g
        self.buf = torch.full((pos,), NAN, dtype=dtype, device=d)
        assert self.buf.data_ptr() % 16 == 0

    def view(self, name):
        pos, rows, cols = self.spans[name]
        return self.buf[pos:pos + rows * cols].view(rows, cols)

    def outside(self):
        """every element of the allocation that belongs to no output: guards and alignment gaps"""
        mask = torch.ones(self.buf.numel(), dtype=torch.bool)
        for pos, rows, cols in self.spans.values():
            mask[pos:pos + rows * cols] = False
        return self.buf.cpu()[mask]


def _operand(t, off, d, behind):
    """t [rows, width] as dense bf16 rows whose first element lies `off` elements into a 16-byte aligned, NaN-filled buffer that
    also holds `behind` NaN rows after the last one"""
    rows, width = t.shape
    buf = torch.full((off + (rows + behind) * width + 8,), NAN, dtype=torch.bfloat16, device=d)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + rows * width].view(rows, width)
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + 2 * off
    return v


def _tables(i, c, d):
    """(p, idx) for the three table slots: each table [TABLE_ROWS + 1, M] with an all-NaN last row, each index array N + PAD_ROWS
    long with every entry past N pointing at that row — a stale index shows as NaN and never leaves the table"""
    N = c["N"]
    p, idx = [None] * 3, [None] * 3
    for slot, tab, ix in zip(c["slots"], i["tables"], i["idx"]):
        t = torch.full((B.TABLE_ROWS + 1, c["M"]), NAN, dtype=torch.bfloat16, device=d)
        t[:B.TABLE_ROWS].copy_(tab)
        full = torch.full((N + B.PAD_ROWS,), B.TABLE_ROWS, dtype=torch.int32, device=d)
        full[:N].copy_(ix)
        assert int(full.min()) >= 0 and int(full.max()) <= B.TABLE_ROWS
        p[slot], idx[slot] = t, full
    return p, idx


def _run_case(name):
    from matdeeplearn_amd import _lib
    d, bf16 = dev(), torch.bfloat16
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    k = B.case(name)
    i, c = k["inputs"], k["spec"]
    N, K, M, act, entry = c["N"], c["K"], c["M"], c["act"], c["entry"]
    x = _operand(i["g"] if c["xact"] else i["x"], c["xoff"], d, B.PAD_ROWS)
    y = _operand(i["y"], c["yoff"], d, B.PAD_ROWS) if c["xact"] else None
    w = _operand(i["w"], c["woff"], d, 8)
    b = _operand(i["b"][None, :], 0, d, 1)[0] if i["b"] is not None else None
    p, idx = _tables(i, c, d)
    rows = _Arena([("out", N + B.PAD_ROWS, M, c["ooff"])], bf16, d)
    out = rows.view("out")
    stats = entry == "stats"
    f32 = _Arena([("sums", B.SUMS_ROWS + 1, M, 0)], torch.float32, d) if stats else None
    sums = f32.view("sums") if stats else None
    nd = torch.tensor([c["nd"]], dtype=torch.int64, device=d) if c["nd"] is not None else None
    # the route this call takes, from the pointers it passes
    al = dict(x_mod16=x.data_ptr() % 16, w_mod4=w.data_ptr() % 4, out_mod2=out.data_ptr() % 2)
    if entry == "wide":
        route = B.wide_route(N, K, M, **al)
    else:
        route = B.lin_route(entry, N, K, M, sum(t is not None for t in p), c["xact"], stats, act=act,
                            y_mod4=0 if y is None else y.data_ptr() % 4, **al)
    assert route == k["route"], (name, route)
    for off, t in ((c["xoff"], x), (c["yoff"], y), (c["woff"], w), (c["ooff"], out)):
        assert t is None or t.data_ptr() % 16 == (2 * off) % 16

    def launch():
        rows.buf.fill_(NAN)
        if stats:
            sums.fill_(NAN)
            sums[:2 * B.REPLICAS].zero_()
            sums[2 * B.REPLICAS:B.SUMS_ROWS].fill_(SENTINEL)
        tabs = (P(p[0]), P(idx[0]), P(p[1]), P(idx[1]), P(p[2]), P(idx[2]))
        if entry == "act":
            rc, what = L.mdl_linear_act(P(x), P(w), P(b), P(out), N, K, M, act, _lib.MDL_BF16, st()), "mdl_linear_act"
        elif entry == "in":
            rc, what = L.mdl_linear_act_in(P(x), P(y), c["xact"], P(w), P(b), P(out), N, K, M, act, _lib.MDL_BF16, st()), "mdl_linear_act_in"
        elif entry == "gather":
            rc, what = L.mdl_linear_gather_act(P(x), P(w), P(b), *tabs, P(out), N, K, M, act, _lib.MDL_BF16, st()), "mdl_linear_gather_act"
        elif entry == "stats":
            rc, what = L.mdl_linear_act_stats(P(x), P(w), P(b), *tabs, P(out), N, K, M, act, P(sums), P(nd), _lib.MDL_BF16, st()), "mdl_linear_act_stats"
        else:
            rc, what = L.mdl_linear_wide(P(x), P(w), P(out), N, K, M, _lib.MDL_BF16, st()), "mdl_linear_wide"
        _lib.check(rc, what)
        torch.cuda.synchronize()
        # what the kernel must not write: the guards and gaps around the output, every row past N
        assert bool(torch.isnan(rows.outside().float()).all()), "a store landed outside the output"
        o = out.cpu().float()
        assert bool(torch.isnan(o[N:]).all()), "an output row past N was written"
        got = dict(out=o[:N].contiguous())
        if stats:
            assert bool(torch.isnan(f32.outside()).all()), "a store landed outside the sums"
            got["sums"] = sums.cpu().clone()
        return got

    got = launch()
    again = launch()
    o = got["out"]
    bad = ~torch.isfinite(o)
    assert not bool(bad.any()), "%s: %d elements of [N, M] are NaN / inf or were left unwritten, first at %s" % (
        name, int(bad.sum()), bad.nonzero()[0].tolist())
    assert torch.equal(o, again["out"]), "two launches differ: the output has no atomics"
    rep = B.judge(o, k)
    line = "[budget] %-18s %-42s ratio %.6f  equal %d/%d" % (name, B.route_label(route), rep["ratio"], int((o == k["model"]["out"]).sum()), o.numel())
    if c["xact"] != 2:
        line += "  single %.4f inside %.4f" % (rep["single"], rep["inside"]) + ("  ssp %.2f u" % rep["ssp_units"] if act == 2 else "")
    chk = sr = None
    if stats:
        s = got["sums"].double()
        n = B.n_true_of(c)
        sh = got["sums"][B.SUMS_ROWS]
        S0, S1 = s[0:2 * B.REPLICAS:2].sum(0), s[1:2 * B.REPLICAS:2].sum(0)
        chk, sr = B.stats_check(o, sh, S0, S1, n), B.stat_ratios(sh, S0, S1, k)
        line += "  stats f0 %.3g f1 %.3g sh %d  mean %.6f var %.6f" % (chk["f0"], chk["f1"], chk["sh_steps"], sr["mean"], sr["var"])
    print(line)
    if c["ints"]:
        assert torch.equal(o, k["model"]["out"]), "integer inputs: the output is exact in any summation order"
    assert rep["ratio"] <= B.ALLOWED["out"], "%s %s: over the budget %.1f: %.4f" % (name, route, B.ALLOWED["out"], rep["ratio"])
    if c["xact"] != 2:
        assert rep["inside"] == 1.0, "%s: %.6f of the elements lie inside their interval of admissible bf16 values" % (name, rep["inside"])
        assert rep["ssp_units"] <= B.SSP_C
    if stats:
        sm = got["sums"]
        assert bool(torch.isfinite(sm).all()) and torch.equal(B.bfr(sh), sh), "the shift row is bf16-valued"
        assert chk["sh_steps"] <= 1, "the stored shift is output row 0 to within one bf16 step"
        used = min(route[7], B.REPLICAS)
        assert float(sm[2 * used:2 * B.REPLICAS].abs().max() if used < B.REPLICAS else 0.0) == 0.0, "a replica no workgroup maps to was written"
        assert bool((sm[2 * B.REPLICAS:B.SUMS_ROWS] == SENTINEL).all()), "the totals rows are the caller's"
        assert chk["f0"] <= 1.0 and chk["f1"] <= 1.0, "%s: the sums are over their derived bounds: %s" % (name, chk)
        assert sr["mean"] <= B.ALLOWED["mean"] and sr["var"] <= B.ALLOWED["var"], (name, sr)
        assert torch.equal(again["sums"][B.SUMS_ROWS], sh), "the shift is the same bits in every launch"


@pytest.mark.parametrize("name", list(B.PLAIN_CASES))
def test_linear_act_forms_through_the_c_abi(name):
    _run_case(name)


@pytest.mark.parametrize("name", list(B.GATHER_CASES))
def test_linear_gather_act_through_the_c_abi(name):
    _run_case(name)


@pytest.mark.parametrize("name", list(B.XACT_CASES))
def test_linear_act_in_through_the_c_abi(name):
    _run_case(name)


@pytest.mark.parametrize("name", list(B.STATS_CASES))
def test_linear_act_stats_through_the_c_abi(name):
    _run_case(name)


@pytest.mark.parametrize("name", list(B.WIDE_CASES))
def test_linear_wide_through_the_c_abi(name):
    _run_case(name)


def test_the_entry_points_refuse_what_they_cannot_do():
    """the return code, the error text and that nothing was written, for every shape, table count and pointer the five entry points
    refuse; N = 0 is MDL_OK and writes nothing either.  The mirror gives the same verdict for each."""
    from matdeeplearn_amd import _lib
    d, bf16 = dev(), torch.bfloat16
    L, st = _lib.lib(), _lib.stream
    V = ctypes.c_void_p
    g = torch.Generator().manual_seed(5)
    N = 100
    x = _operand(B.bfr(torch.randn(N, 260, generator=g)), 0, d, B.PAD_ROWS)
    y = _operand(B.bfr(torch.randn(N, 260, generator=g)), 0, d, B.PAD_ROWS)
    w = _operand(B.bfr(torch.randn(164, 260, generator=g)), 0, d, 8)
    b = _operand(B.bfr(torch.randn(1, 164, generator=g)), 0, d, 1)
    tab = torch.zeros(B.TABLE_ROWS + 1, 164, dtype=bf16, device=d)
    ix = torch.zeros(N + B.PAD_ROWS, dtype=torch.int32, device=d)
    rows = _Arena([("out", N + B.PAD_ROWS, 164, 0)], bf16, d)
    f32 = _Arena([("sums", B.SUMS_ROWS + 1, 164, 0)], torch.float32, d)
    X, Y, Wp, Bp, T, I, O, S = (t.data_ptr() for t in (x, y, w, b, tab, ix, rows.view("out"), f32.view("sums")))
    BF = _lib.MDL_BF16

    def act(K, M, n=N, x=X, w=Wp, o=O):
        return L.mdl_linear_act(V(x), V(w), V(Bp), V(o), n, K, M, 1, BF, st()), B.lin_route("act", n, K, M, x_mod16=x % 16, w_mod4=w % 4, out_mod2=o % 2)

    def inn(K, M, xact=0, n=N, x=X, w=Wp, yp=Y):
        return (L.mdl_linear_act_in(V(x), V(yp), xact, V(w), V(Bp), V(O), n, K, M, 1, BF, st()),
                B.lin_route("in", n, K, M, 0, xact, x_mod16=x % 16, w_mod4=w % 4, y_mod4=yp % 4))

    def slots(tables, orphan):
        a = []
        for s in range(3):
            a += [V(T) if s < tables else None, V(I) if s < tables and not (orphan and s == tables - 1) else None]
        return a

    def gather(K, M, tables, orphan=False):
        return (L.mdl_linear_gather_act(V(X), V(Wp), V(Bp), *slots(tables, orphan), V(O), N, K, M, 1, BF, st()),
                B.lin_route("gather", N, K, M, tables, orphan=orphan))

    def stats(K, M, tables=0, orphan=False, n=N, x=X, w=Wp, o=O):
        return (L.mdl_linear_act_stats(V(x), V(w), V(Bp), *slots(tables, orphan), V(o), n, K, M, 1, V(S), None, BF, st()),
                B.lin_route("stats", n, K, M, tables, 0, True, orphan=orphan, x_mod16=x % 16, w_mod4=w % 4, out_mod2=o % 2))

    def wide(K, M, n=N, x=X, w=Wp, o=O):
        return L.mdl_linear_wide(V(x), V(w), V(o), n, K, M, BF, st()), B.wide_route(n, K, M, x_mod16=x % 16, w_mod4=w % 4, out_mod2=o % 2)

    shape = "need even 4<=K<=256 and 1<=M<=160 (K<=160 when M>128)"
    sshape = "mdl_linear_act_stats: need even 4<=K<=160 and even 34<=M<=160 (<=128 with tables)"
    refused = [
        (lambda: act(63, 32), -2, shape), (lambda: act(2, 32), -2, shape), (lambda: act(258, 32), -2, shape),
        (lambda: act(64, 161), -2, shape), (lambda: act(162, 130), -2, shape),
        (lambda: inn(63, 32), -2, shape), (lambda: inn(2, 32, 1), -2, shape), (lambda: inn(258, 32, 2), -2, shape),
        (lambda: inn(64, 161), -2, shape), (lambda: inn(162, 130), -2, shape),
        (lambda: gather(64, 130, 1), -2, "gathered tables need M <= 128 (got 130)"), (lambda: gather(64, 130, 3), -2, "gathered tables need M <= 128"),
        (lambda: gather(64, 64, 2, orphan=True), -1, "mdl_linear_gather_act: table without index"),
        (lambda: stats(64, 64, 2, orphan=True), -1, "mdl_linear_act_stats: table without index"),
        (lambda: stats(64, 32), -2, sshape), (lambda: stats(64, 35), -2, sshape), (lambda: stats(162, 64), -2, sshape),
        (lambda: stats(64, 130, 2), -2, sshape),
        (lambda: stats(64, 64, 1), -2, "mdl_linear_act_stats: unsupported shape (K=64 M=64 tables=1)"),
        (lambda: stats(64, 64, 3), -2, "mdl_linear_act_stats: unsupported shape (K=64 M=64 tables=3)"),
        (lambda: wide(162, 700), -2, "mdl_linear_wide: need even 4<=K<=160"), (lambda: wide(63, 700), -2, "mdl_linear_wide: need even 4<=K<=160"),
        # each pointer an entry point names
        (lambda: act(64, 32, x=X + 4), -1, "mdl_linear_act: misaligned pointer"), (lambda: act(64, 32, w=Wp + 2), -1, "mdl_linear_act: misaligned pointer"),
        (lambda: act(64, 32, o=O + 1), -1, "mdl_linear_act: misaligned pointer"),
        (lambda: inn(64, 32, x=X + 2), -1, "mdl_linear_act_in: misaligned pointer"), (lambda: inn(64, 32, w=Wp + 2), -1, "mdl_linear_act_in: misaligned pointer"),
        (lambda: inn(64, 32, 1, yp=Y + 2), -1, "mdl_linear_act_in: xact must be"), (lambda: inn(64, 32, 3), -1, "mdl_linear_act_in: xact must be"),
        (lambda: stats(64, 64, x=X + 4), -1, "mdl_linear_act_stats: misaligned pointer"), (lambda: stats(64, 64, w=Wp + 2), -1, "mdl_linear_act_stats: misaligned pointer"),
        (lambda: stats(64, 64, o=O + 1), -1, "mdl_linear_act_stats: misaligned pointer"),
        (lambda: wide(64, 700, x=X + 4), -1, "mdl_linear_wide: misaligned pointer"), (lambda: wide(64, 700, w=Wp + 2), -1, "mdl_linear_wide: misaligned pointer"),
        (lambda: wide(64, 700, o=O + 1), -1, "mdl_linear_wide: misaligned pointer"),
    ]
    for n, (call, code, text) in enumerate(refused):
        rc, route = call()
        err = L.mdl_last_error_string().decode()
        assert rc == code and text in err, (n, rc, err)
        assert route[0] == {-1: "arg", -2: "unsupp"}[code] and route[1] in err, (n, route, err)
    for call in (lambda: act(64, 32, n=0), lambda: inn(64, 32, 1, n=0), lambda: stats(64, 64, n=0), lambda: wide(64, 700, n=0)):
        rc, route = call()
        assert rc == 0 and route == ("empty",)
    torch.cuda.synchronize()
    assert bool(torch.isnan(rows.buf).all()) and bool(torch.isnan(f32.buf).all()), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------
# layer level
# ---------------------------------------------------------------------------------------------
def _count(monkeypatch, seen):
    """wrap the entry points of csrc/linear.hip (and the BatchNorm statistics kernel) on the loaded library: every launch is recorded
    as (entry point, K, M, tables[, xact])"""
    from matdeeplearn_amd import _lib
    L = _lib.lib()
    orig = {n: getattr(L, n) for n in ("mdl_linear_act", "mdl_linear_act_in", "mdl_linear_gather_act", "mdl_linear_act_stats",
                                       "mdl_linear_wide", "mdl_bn_stats_n")}
    ntab = lambda a: sum(1 for t in a if t is not None and getattr(t, "value", t) is not None)

    def act(x, w, b, out, N, K, M, a, dt, s):
        seen.append(("mdl_linear_act", K, M, 0))
        return orig["mdl_linear_act"](x, w, b, out, N, K, M, a, dt, s)

    def act_in(x, y, xact, w, b, out, N, K, M, a, dt, s):
        seen.append(("mdl_linear_act_in", K, M, 0, xact))
        return orig["mdl_linear_act_in"](x, y, xact, w, b, out, N, K, M, a, dt, s)

    def gather(x, w, b, p1, i1, p2, i2, p3, i3, out, N, K, M, a, dt, s):
        seen.append(("mdl_linear_gather_act", K, M, ntab((p1, p2, p3))))
        return orig["mdl_linear_gather_act"](x, w, b, p1, i1, p2, i2, p3, i3, out, N, K, M, a, dt, s)

    def stats(x, w, b, p1, i1, p2, i2, p3, i3, out, N, K, M, a, sums, nd, dt, s):
        seen.append(("mdl_linear_act_stats", K, M, ntab((p1, p2, p3))))
        return orig["mdl_linear_act_stats"](x, w, b, p1, i1, p2, i2, p3, i3, out, N, K, M, a, sums, nd, dt, s)

    def wide(x, w, out, N, K, M, dt, s):
        seen.append(("mdl_linear_wide", K, M, 0))
        return orig["mdl_linear_wide"](x, w, out, N, K, M, dt, s)

    def bn_stats(x, sums, N, C, nd, fl, s):
        seen.append(("mdl_bn_stats_n", 0, C, 0))
        return orig["mdl_bn_stats_n"](x, sums, N, C, nd, fl, s)
    for n, f in (("mdl_linear_act", act), ("mdl_linear_act_in", act_in), ("mdl_linear_gather_act", gather), ("mdl_linear_act_stats", stats),
                 ("mdl_linear_wide", wide), ("mdl_bn_stats_n", bn_stats)):
        monkeypatch.setattr(L, n, f)


@pytest.mark.parametrize("name", list(B.LAYER_CASES))
def test_layer_forward(name, monkeypatch):
    """ops.linear_act / linear_gather_act / linear_relu_bn / matmul_wide in bf16 on fp32 master weights against the fp64 layer; the
    launches that served the forward are counted, each with its entry point and (K, M, tables).
    linear_relu_bn: z, running_mean and running_var against an fp64 BatchNorm of the MODEL's rounded y.  What they may differ by
    is reasoned, not measured: z is one bf16 rounding of the normalised value (relative 2^-8), the kernel's y may differ from
    the model's in an element by one bf16 step (gamma rstd step in z: the interval of such an element holds two values), and one
    such step in a column moves the mean by step / N and the variance by 2 max|y - mean| step / N; the fp32 sums carry the (n + 18) u of the statistics bound
    (32 times that for the variance, whose two terms are up to 10 var each about a shift 3 sigma off the mean); z inherits the
    movement of mean and variance, and the fp32 arithmetic of the apply kernel is 2^-16 (1 + |z|)."""
    from matdeeplearn_amd import ops
    d, bf16 = dev(), torch.bfloat16
    op, N, K, M, act, tables, det, calls = B.LAYER_CASES[name]
    k = B.layer_case(name)
    i = k["inputs"]
    seen = []
    _count(monkeypatch, seen)
    x = i["x"].to(d).to(bf16).requires_grad_(True)
    gath = [(t.to(d).to(bf16), ix.to(d)) for t, ix in zip(i["tables"], i["idx"])]
    if op == "matmul_wide":
        out = ops.matmul_wide(x, i["w"].t().contiguous().to(d).to(bf16))
    else:
        w, b = i["w"].to(d).requires_grad_(True), i["b"].to(d).requires_grad_(True)
        if op == "linear_act":
            out = ops.linear_act(x, w, b, act)
        elif op == "linear_gather_act":
            out = ops.linear_gather_act(x, w, b, act, gath)
        else:
            gen = torch.Generator().manual_seed(77)
            gamma, beta = torch.rand(M, generator=gen) + 0.5, torch.randn(M, generator=gen) * 0.2
            rm, rv = torch.zeros(M, device=d), torch.ones(M, device=d)
            eps, mom = 1e-5, 0.1
            assert ops.linear_relu_bn_ok(x, w, True, gath or None)
            with ops.deterministic(det):
                out = ops.linear_relu_bn(x, w, b, None, gamma.to(d), beta.to(d), rm, rv, eps, mom, gath or None)
    torch.cuda.synchronize()
    assert seen == calls, seen
    assert out.dtype == bf16 and tuple(out.shape) == (N, M)
    got = out.detach().float().cpu()
    assert bool(torch.isfinite(got).all())
    if op != "linear_relu_bn":
        rep = B.judge(got, k)
        print("[budget] %-18s %-42s ratio %.4f  equal %d/%d  single %.4f inside %.4f" % (
            name, "%d launch(es): %s" % (len(seen), seen[0][0]), rep["ratio"], int((got == k["model"]["out"]).sum()), got.numel(), rep["single"], rep["inside"]))
        assert rep["ratio"] <= B.ALLOWED["out"] and rep["inside"] == 1.0 and rep["ssp_units"] <= B.SSP_C, (name, rep)
        return
    ym = k["model"]["out"]
    z64, rm64, rv64 = B.batchnorm64(ym, gamma, beta, eps, mom)
    step = (B.bf_step(ym, 1) - ym).double()
    mean, var = ym.double().mean(0), ym.double().var(0, unbiased=False)
    rstd = 1.0 / torch.sqrt(var + eps)
    dm = step.max(0).values / N                                                         # a one-step flip in a column: the mean ...
    dv = 2 * (ym.double() - mean).abs().max(0).values * step.max(0).values / N          # ... and the variance
    fm, fv = (N + 18) * B.U * (mean.abs() + var.sqrt()), 32 * (N + 19) * B.U * var      # fp32 sums about a shift up to 3 sigma off the mean
    tol_m = mom * (dm + fm)
    tol_v = mom * (dv + fv) * N / (N - 1)
    tol_z = (2.0 ** -8 * z64.abs() + gamma.double().abs() * rstd * (step + dm + fm) + (z64 - beta.double()).abs() * 0.5 * (dv + fv) / (var + eps)
             + 2.0 ** -16 * (1 + z64.abs()))
    ez, em, ev = (got.double() - z64).abs(), (rm.cpu().double() - rm64).abs(), (rv.cpu().double() - rv64).abs()
    print("[budget] %-18s %-42s z %.3f  running_mean %.2g  running_var %.2g of their tolerances" % (
        name, "%d launch(es): %s" % (len(seen), seen[0][0]), float((ez / tol_z).max()), float((em / tol_m.clamp(min=1e-30)).max()),
        float((ev / tol_v.clamp(min=1e-30)).max())))
    assert bool((ez <= tol_z).all()) and bool((em <= tol_m).all()) and bool((ev <= tol_v).all()), name


@pytest.mark.parametrize("name", list(B.DX_CASES))
def test_the_input_gradient_of_a_narrow_activated_layer_comes_from_linear_act_in(name, monkeypatch):
    """linear_act(..., "relu" / "ssp") with M = 20, K = 64 and an input gradient wanted: M < 34 keeps the one-pass dense backward
    away, dW / db take the TN GEMM with the activation staging, and dX = (g .* act'(y)) W must come from mdl_linear_act_in with
    kernel K = 20 and kernel M = 64 — the route the dense-backward suite does not reach.  y is the layer's own output."""
    from matdeeplearn_amd import ops
    d, bf16 = dev(), torch.bfloat16
    Ld = B.dx_layer(name)
    seen = []
    _count(monkeypatch, seen)
    x = Ld["x"].to(d).to(bf16).requires_grad_(True)
    w, b = Ld["w"].to(d).requires_grad_(True), Ld["b"].to(d).requires_grad_(True)
    out = ops.linear_act(x, w, b, Ld["act"])
    (out.float() * Ld["gout"].to(d)).sum().backward()
    torch.cuda.synchronize()
    assert seen == [("mdl_linear_act", B.DX_K, B.DX_M, 0), ("mdl_linear_act_in", B.DX_M, B.DX_K, 0, Ld["code"])], seen
    k = B.dx_from(name, out.detach().float().cpu())
    got = x.grad.float().cpu()
    rep = B.judge(got, k)
    print("[budget] %-18s %-42s ratio %.4f  equal %d/%d" % (name, "dX: mdl_linear_act_in", rep["ratio"], int((got == k["model"]["out"]).sum()), got.numel()))
    assert rep["ratio"] <= B.ALLOWED["out"], (name, rep)
    if Ld["code"] == 1:
        assert rep["inside"] == 1.0, rep
