"""The fused MLP head (csrc/mlp.hip), the GRU gates (csrc/gru.hip) and the loss (csrc/loss.hip) on the device against the fp64
reference, within the measures of tests/head_budget.py: per row within ALLOWED times the error of the rounding model, every stored
value inside its derived interval, every fp32 sum within its derived bound, integer data bit for bit.  Everything goes through the
C ABI with the operands inside NaN-filled buffers (70 NaN rows behind the last one: a read outside poisons the result) and the
outputs carved out of NaN-filled arenas (what must not be written stays NaN).  Every case is launched twice: what has no atomics
must be bit-equal, and both runs of the atomic dW / db must pass.  The forward is judged layer by layer on the kernel's own stored
input; the backward once on the model's hidden outputs and once chained on the kernel's own.
Layer level: ops.mlp_head / gru_gates / loss issue exactly the native calls they claim and return the C ABI's bits.
test_head_budget_host.py shows that these checks can fail: every mutation of the model breaks the measure that owns it."""
import ctypes

import pytest
import torch

import head_budget as B

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


class _Arena:
    """outputs of one dtype carved out of ONE NaN-filled allocation, GUARD bytes behind each, every output on a 16-byte boundary"""

    def __init__(self, specs, dtype, d):
        size = torch.empty(0, dtype=dtype).element_size()
        g, al = B.GUARD // size, 16 // size
        self.spans, pos = {}, g
        for name, rows, cols in specs:
            pos = (pos + al - 1) // al * al
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
        return self.buf.cpu()[mask].float()


def _operand(t, dtype, d, off=0):
    """t [n, C] (a vector: one row) as the first rows of a NaN-filled buffer of n + PAD_ROWS rows whose first element lies `off`
    elements past a 16-byte boundary: everything behind the data is NaN"""
    t = t.view(1, -1) if t.dim() == 1 else t
    n, C = t.shape
    buf = torch.full((off + (n + B.PAD_ROWS) * C + 8,), NAN, dtype=dtype, device=d)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + n * C].view(n, C)
    v.copy_(t)
    return v


def _all_nan(t):
    return bool(torch.isnan(t).all())


def _parr(ts):
    return (ctypes.c_void_p * max(len(ts), 1))(*[None if t is None else (t if isinstance(t, int) else t.data_ptr()) for t in ts])


# ---------------------------------------------------------------------------------------------
# MLP head
# ---------------------------------------------------------------------------------------------
class _Mlp:
    """one case's operands on the device and its output arenas"""

    def __init__(self, i, c):
        from matdeeplearn_amd import _lib
        d, bf16 = dev(), torch.bfloat16
        self.i, self.c, self.d = i, c, d
        N, NL, M, Ks = i["N"], i["NL"], i["M"], i["Ks"]
        self.x = _operand(i["x"], bf16, d)
        self.w = [_operand(w, bf16, d) for w in i["w"]]
        self.b = [None if b is None else _operand(b, bf16, d) for b in i["b"]]
        self.gy = _operand(i["gy"], torch.float32 if i["f32io"] else bf16, d, off=c["gy_off"])
        self.io = _lib.MDL_MLP_F32_IO if i["f32io"] else 0
        rows = N + B.PAD_ROWS
        self.lp = _Arena([("h%d" % l, rows, M[l]) for l in range(NL) if not (i["f32io"] and l == NL - 1)] + [("dx", rows, i["K0"])], bf16, d)
        self.f32 = _Arena(([("y", rows, M[-1])] if i["f32io"] else []) + [("dw%d" % l, M[l] + 3, Ks[l]) for l in range(NL)]
                          + [("db%d" % l, 1, M[l]) for l in range(NL)], torch.float32, d)
        self.h = [self.f32.view("y") if (i["f32io"] and l == NL - 1) else self.lp.view("h%d" % l) for l in range(NL)]
        self.Ma = (ctypes.c_int * NL)(*M)
        # the true addresses, through the mirror: the call is one the entry points take, on the route the case is pinned to
        assert self.gy.data_ptr() % 4 == (2 if (c["gy_off"] % 2 and not i["f32io"]) else 0)
        for direction in ("fwd", "bwd"):
            assert B.mlp_accepts(direction, N, i["K0"], M, f32io=i["f32io"], x=self.x.data_ptr(), w=[w.data_ptr() for w in self.w],
                                 h=[h.data_ptr() for h in self.h], gy=self.gy.data_ptr(), dw=[self.f32.view("dw%d" % l).data_ptr() for l in range(NL)]) == B.OK

    def forward(self):
        """the stored outputs of every layer on the CPU [NL], after the guard checks"""
        from matdeeplearn_amd import _lib
        L, P, st = _lib.lib(), _lib.ptr, _lib.stream
        i, N = self.i, self.i["N"]
        self.lp.buf.fill_(NAN), self.f32.buf.fill_(NAN)
        _lib.check(L.mdl_mlp_head_fwd(P(self.x), _parr(self.w), _parr(self.b), _parr(self.h), N, i["K0"], i["NL"], self.Ma, _lib.MDL_BF16 | self.io,
                                      st()), "mdl_mlp_head_fwd")
        torch.cuda.synchronize()
        assert _all_nan(self.lp.outside()) and _all_nan(self.f32.outside()), "a store landed outside the outputs"
        assert _all_nan(self.lp.view("dx")) and all(_all_nan(self.f32.view("dw%d" % l)) for l in range(i["NL"])), "the forward wrote a gradient"
        out = [h.cpu().float() for h in self.h]
        for l, o in enumerate(out):
            assert _all_nan(o[N:]), "layer %d: a row behind the last one was written" % l
        return [o[:N].contiguous() for o in out]

    def backward(self, hs, det):
        """dict(dx, dw, db) on the CPU from the hidden outputs hs (CPU, fp32 holding bf16 values), after the guard checks"""
        from matdeeplearn_amd import _lib
        L, P, st = _lib.lib(), _lib.ptr, _lib.stream
        i, N, NL, M = self.i, self.i["N"], self.i["NL"], self.i["M"]
        hdev = [_operand(h, torch.bfloat16, self.d) for h in hs]
        self.lp.buf.fill_(NAN), self.f32.buf.fill_(NAN)
        dw = [self.f32.view("dw%d" % l)[:M[l]] for l in range(NL)]
        db = [None if l in i["nobias"] else self.f32.view("db%d" % l) for l in range(NL)]
        for t in dw + [t for t in db if t is not None]:
            t.zero_()                                                # the caller zero-fills what the kernel adds to
        dx = self.lp.view("dx") if i["want_dx"] else None
        flag = _lib.MDL_DETERMINISTIC if det else 0
        _lib.check(L.mdl_mlp_head_bwd(P(self.x), _parr(self.w), _parr(hdev + [None]), P(self.gy), P(dx), _parr(dw), _parr(db), N, i["K0"], NL, self.Ma,
                                      _lib.MDL_BF16 | self.io | flag, st()), "mdl_mlp_head_bwd")
        torch.cuda.synchronize()
        assert _all_nan(self.lp.outside()) and _all_nan(self.f32.outside()), "a store landed outside the outputs"
        assert all(_all_nan(h) for name, h in zip(range(NL), self.h)), "the backward wrote a forward output"
        for l in range(NL):
            assert _all_nan(self.f32.view("dw%d" % l)[M[l]:]), "dw%d: a row behind the last one was written" % l
            assert db[l] is not None or _all_nan(self.f32.view("db%d" % l)), "db%d was written without being asked for" % l
        got = dict(dw=[t.cpu().clone() for t in dw], db=[None if t is None else t.cpu().view(-1).clone() for t in db], dx=None)
        if dx is None:
            assert _all_nan(self.lp.view("dx")), "dx was written without being asked for"
        else:
            o = dx.cpu().float()
            assert _all_nan(o[N:]), "dx: a row behind the last one was written"
            got["dx"] = o[:N].contiguous()
        return got


def _same(a, b):
    return all((x is None and y is None) or torch.equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("name", list(B.MLP_CASES))
def test_mlp_head_through_the_c_abi(name):
    k = B.mlp_case(name)
    i, c = k["inputs"], k["spec"]
    routes = (B.mlp_route(i["N"], i["K0"], i["M"], i["f32io"], c["det"], "fwd"), B.mlp_route(i["N"], i["K0"], i["M"], i["f32io"], c["det"], "bwd"))
    assert routes == k["routes"] and (not c["det"] or routes[1][1] == 1), (name, routes)
    run = _Mlp(i, c)
    layers = run.forward()
    assert _same(run.forward(), layers), "the forward has no atomics: two runs are bit-equal"
    fails, rep = B.mlp_judge_fwd(i, layers)
    print("[budget] %-18s fwd grid %d trips %d | bwd grid %d trips %d gy %s   %s   single %s" % (
        name, routes[0][1], routes[0][2], routes[1][1], routes[1][2], routes[1][4], B.f3(rep["ratios"]), " ".join("%.3f" % v for v in rep["single"])))
    assert not fails, (name, fails)
    own = layers[:-1]
    mod_h = k["model_h"][:-1]
    for label, hs in (("model h", mod_h), ("own h", own)):
        mr = (B.mlp_backward(i, hs), B.mlp_backward(i, hs, torch.float64, rounded=False))
        a, b = run.backward(hs, c["det"]), run.backward(hs, c["det"])
        assert (a["dx"] is None and b["dx"] is None) or torch.equal(a["dx"], b["dx"]), "dx has no atomics: two runs are bit-equal"
        if c["det"]:
            assert _same(a["dw"], b["dw"]) and _same(a["db"], b["db"]), "MDL_DETERMINISTIC is not reproducible"
        worst = {}
        for got in (a, b):
            fails, repb = B.mlp_judge_bwd(i, hs, got, mod_ref=mr)
            for q, v in list(repb["ratios"].items()) + [("bound_" + q, v) for q, v in repb["bound"].items()]:
                worst[q] = max(worst.get(q, 0.0), v)
            assert not fails, (name, label, fails)
        print("[budget] %-18s bwd on %-7s %s   agree %s" % (name, label, B.f3(worst), repb["agree"]))


def test_mlp_head_refuses_what_it_cannot_do():
    """the return code of every refused call as the mirror gives it for the true addresses, and nothing written; N = 0 is MDL_OK and
    writes nothing either"""
    from matdeeplearn_amd import _lib
    d, bf16 = dev(), torch.bfloat16
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    N, K0, M = 5, 64, [64, 3]
    x = _operand(torch.randn(N, K0), bf16, d)
    w = [_operand(torch.randn(64, 64), bf16, d), _operand(torch.randn(3, 64), bf16, d)]
    hid = _operand(torch.randn(N, 64), bf16, d)
    gy, gy32 = _operand(torch.randn(N, 3), bf16, d), _operand(torch.randn(N, 3), torch.float32, d)
    lp = _Arena([("h0", N, 64), ("h1", N, 3), ("dx", N, K0)], bf16, d)
    f32 = _Arena([("dw0", 64, 64), ("dw1", 3, 64), ("db0", 1, 64), ("db1", 1, 3)], torch.float32, d)
    a = lambda t: t.data_ptr()
    ok = dict(N=N, K0=K0, M=M, dtype="bf16", f32io=False, x=a(x), w=[a(w[0]), a(w[1])], h=[a(lp.view("h0")), a(lp.view("h1"))], gy=a(gy),
              dw=[a(f32.view("dw0")), a(f32.view("dw1"))])
    both = [dict(M=[]), dict(M=[2] * 5, w=[a(w[0])] * 5, h=[a(hid)] * 5, dw=[a(f32.view("dw0"))] * 5), dict(K0=63), dict(K0=66), dict(M=[63, 3]),
            dict(M=[64, 65]), dict(M=[65, 2]), dict(w=[a(w[0]), None]), dict(w=[a(w[0]) + 2, a(w[1])]), dict(x=a(x) + 2), dict(x=None), dict(dtype="f32"),
            dict(N=-1), dict(N=0)]
    bwd_only = [dict(gy=None), dict(gy=a(gy) + 1), dict(gy=a(gy32) + 2, f32io=True), dict(M=[64, 2], gy=a(gy) + 2), dict(dw=[a(f32.view("dw0")), None]),
                dict(h=[None, None]), dict(h=[a(hid) + 2, None])]
    fwd_only = [dict(h=[a(lp.view("h0")), None])]
    codes = set()
    for direction, muts in (("fwd", both + fwd_only), ("bwd", both + bwd_only)):
        for m in muts:
            kw = dict(ok, **m)
            if direction == "bwd" and "h" not in m:
                kw["h"] = [a(hid), None]
            want = B.mlp_accepts(direction, **kw)
            assert (want == B.OK) == (kw["N"] == 0), (direction, m)
            NL = len(kw["M"])
            Ma = (ctypes.c_int * max(NL, 1))(*kw["M"])
            code = (_lib.MDL_BF16 if kw["dtype"] == "bf16" else _lib.MDL_F32) | (_lib.MDL_MLP_F32_IO if kw["f32io"] else 0)
            vp = lambda v: None if v is None else ctypes.c_void_p(v)
            if direction == "fwd":
                rc = L.mdl_mlp_head_fwd(vp(kw["x"]), _parr(kw["w"]), _parr([None] * NL), _parr(kw["h"]), kw["N"], kw["K0"], NL, Ma, code, st())
            else:
                rc = L.mdl_mlp_head_bwd(vp(kw["x"]), _parr(kw["w"]), _parr(kw["h"]), vp(kw["gy"]), P(lp.view("dx")), _parr(kw["dw"]),
                                        _parr([a(f32.view("db0")), a(f32.view("db1"))] + [None] * 3), kw["N"], kw["K0"], NL, Ma, code, st())
            assert rc == want, (direction, m, rc, L.mdl_last_error_string())
            codes.add(rc)
    torch.cuda.synchronize()
    assert codes == {B.OK, B.E_ARG, B.E_UNSUPP}
    assert _all_nan(lp.buf) and _all_nan(f32.buf), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------
# GRU gates
# ---------------------------------------------------------------------------------------------
def _gru_launch(i, c, routes=None):
    """forward and backward of one step through the two entry points; dict of outputs on the CPU after the guard checks"""
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    tdt, dcode = (torch.bfloat16, _lib.MDL_BF16) if i["bf16"] else (torch.float32, _lib.MDL_F32)
    N, C, off = i["N"], i["C"], c["off"]
    gi, gh = _operand(i["gi"], tdt, d, off.get("gi", 0)), _operand(i["gh"], tdt, d, off.get("gh", 0))
    h = _operand(i["h"], torch.float32, d, off.get("h", 0))
    g_h = None if i["g_h"] is None else _operand(i["g_h"], torch.float32, d, off.get("g_h", 0))
    g_lp = None if i["g_lp"] is None else _operand(i["g_lp"], tdt, d, off.get("g_lp", 0))
    rows = N + B.PAD_ROWS
    lp = _Arena([("out_lp", rows, C), ("dgi", rows, 3 * C), ("dgh", rows, 3 * C)], tdt, d)
    f32 = _Arena([("h_out", rows, C), ("dh", rows, C)], torch.float32, d)
    out_lp = lp.view("out_lp") if i["want_out_lp"] else None
    adr = lambda t: None if t is None else t.data_ptr()
    base = dict(gi=adr(gi), gh=adr(gh), out_lp=adr(out_lp), g_lp=adr(g_lp), dgi=adr(lp.view("dgi")), dgh=adr(lp.view("dgh")), h=adr(h),
                h_out=adr(f32.view("h_out")), dh=adr(f32.view("dh")), g_h=adr(g_h))
    true_routes = B.gru_case_routes(c, base)
    assert routes is None or true_routes == routes, (true_routes, routes)

    def run():
        lp.buf.fill_(NAN), f32.buf.fill_(NAN)
        _lib.check(L.mdl_gru_gates_fwd(P(gi), P(gh), P(h), P(f32.view("h_out")), P(out_lp), N, C, dcode, st()), "mdl_gru_gates_fwd")
        torch.cuda.synchronize()
        assert _all_nan(lp.view("dgi")) and _all_nan(lp.view("dgh")) and _all_nan(f32.view("dh")), "the forward wrote a gradient"
        assert out_lp is not None or _all_nan(lp.view("out_lp")), "out_lp was written without being asked for"
        _lib.check(L.mdl_gru_gates_bwd(P(gi), P(gh), P(h), P(g_h), P(g_lp), P(lp.view("dgi")), P(lp.view("dgh")), P(f32.view("dh")), N, C, dcode, st()),
                   "mdl_gru_gates_bwd")
        torch.cuda.synchronize()
        assert _all_nan(lp.outside()) and _all_nan(f32.outside()), "a store landed outside the outputs"
        got = {}
        for q, ar in (("h_out", f32), ("dh", f32), ("dgi", lp), ("dgh", lp)) + ((("out_lp", lp),) if out_lp is not None else ()):
            o = ar.view(q).cpu().float()
            assert _all_nan(o[N:]), "%s: a row behind the last one was written" % q
            got[q] = o[:N].contiguous()
        return got
    got, again = run(), run()
    assert all(torch.equal(got[q], again[q]) for q in got), "no atomics: two runs are bit-equal"
    return got, true_routes


@pytest.mark.parametrize("name", list(B.GRU_CASES))
def test_gru_gates_through_the_c_abi(name):
    k = B.gru_case(name)
    got, routes = _gru_launch(k["inputs"], k["spec"], k["routes"])
    fails, rat = B.gru_judge(k["inputs"], got, k["model"], k["ref"])
    print("[budget] %-18s fwd W%d grid %d trips %d | bwd W%d grid %d trips %d   %s" % ((name,) + routes[0] + routes[1] + (B.f3(rat),)))
    assert not fails, (name, fails)


def test_gru_gates_refuse_what_they_cannot_do():
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    N, C = 5, 8
    gi, gh, h, g = torch.randn(N, 3 * C, device=d), torch.randn(N, 3 * C, device=d), torch.randn(N, C, device=d), torch.randn(N, C, device=d)
    f32 = _Arena([("h_out", N, C), ("out", N, C), ("dgi", N, 3 * C), ("dgh", N, 3 * C), ("dh", N, C)], torch.float32, d)
    v = f32.view
    fwd = lambda gi_=gi, C_=C, dt=_lib.MDL_F32, n=N: L.mdl_gru_gates_fwd(P(gi_), P(gh), P(h), P(v("h_out")), P(v("out")), n, C_, dt, st())
    bwd = lambda gi_=gi, C_=C, dt=_lib.MDL_F32, g_=g, dgi=v("dgi"), n=N: L.mdl_gru_gates_bwd(P(gi_), P(gh), P(h), P(g_), None, P(dgi), P(v("dgh")), P(v("dh")), n, C_, dt, st())
    for f in (fwd, bwd):
        assert f(dt=7) == B.E_UNSUPP and f(C_=0) == B.E_ARG and f(C_=65537) == B.E_ARG and f(gi_=None) == B.E_ARG and f(n=-1) == B.E_ARG
        assert f(n=0) == B.OK
    assert bwd(g_=None) == B.E_ARG and bwd(dgi=None) == B.E_ARG
    assert L.mdl_gru_gates_fwd(P(gi), P(gh), P(h), None, None, N, C, _lib.MDL_F32, st()) == B.E_ARG
    torch.cuda.synchronize()
    assert _all_nan(f32.buf), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------
# loss
# ---------------------------------------------------------------------------------------------
def _loss_launch(i, grad_off):
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    n, nt = i["n"], i["n_total"]
    p, y = _operand(i["p"], torch.float32, d).view(-1), _operand(i["y"], torch.float32, d).view(-1)
    if grad_off:
        ar = _Arena([("out", 1, 1 + nt)], torch.float32, d)          # [loss | gradient]: the gradient one float past a 16-byte boundary
        loss, grad = ar.view("out").view(-1)[:1], ar.view("out").view(-1)[1:]
        assert grad.data_ptr() % 16 == 4
    else:
        ar = _Arena([("loss", 1, 1), ("grad", 1, nt)], torch.float32, d)
        loss, grad = ar.view("loss").view(-1), ar.view("grad").view(-1)

    def run():
        ar.buf.fill_(NAN)
        if nt == n:
            _lib.check(L.mdl_loss_fwd_bwd(P(p), P(y), n, i["kind"], P(loss), P(grad), st()), "mdl_loss_fwd_bwd")
        else:
            _lib.check(L.mdl_loss_fwd_bwd_rows(P(p), P(y), n, nt, i["kind"], P(loss), P(grad), st()), "mdl_loss_fwd_bwd_rows")
        torch.cuda.synchronize()
        assert _all_nan(ar.outside()), "a store landed outside the outputs"
        return dict(loss=loss.cpu().clone(), grad=grad.cpu().clone())
    got, again = run(), run()
    assert torch.equal(got["loss"], again["loss"]) and torch.equal(got["grad"], again["grad"]), "one workgroup, a fixed order: bit-equal"
    return got


@pytest.mark.parametrize("name", list(B.LOSS_CASES))
def test_loss_through_the_c_abi(name):
    k = B.loss_case(name)
    got = _loss_launch(k["inputs"], k["spec"]["grad_off"])
    fails, rep = B.loss_judge(k["inputs"], got, k["model"], k["ref"])
    print("[budget] %-18s %s" % (name, B.f3(rep)))
    assert not fails, (name, fails)


def test_loss_refuses_what_it_cannot_do():
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    n = 100
    p, y = torch.randn(n, device=d), torch.randn(n, device=d)
    ar = _Arena([("loss", 1, 1), ("grad", 1, n)], torch.float32, d)
    lo, gr = ar.view("loss"), ar.view("grad")
    plain = lambda p_=p, y_=y, n_=n, kind=0, lo_=lo, gr_=gr: L.mdl_loss_fwd_bwd(P(p_), P(y_), n_, kind, P(lo_), P(gr_), st())
    rows = lambda p_=p, y_=y, n_=n, nt=n, kind=0, lo_=lo, gr_=gr: L.mdl_loss_fwd_bwd_rows(P(p_), P(y_), n_, nt, kind, P(lo_), P(gr_), st())
    for f in (plain, rows):
        assert f(n_=0) == B.E_ARG and f(kind=2) == B.E_UNSUPP and f(kind=-1) == B.E_UNSUPP
        assert f(p_=None) == B.E_ARG and f(y_=None) == B.E_ARG and f(lo_=None) == B.E_ARG and f(gr_=None) == B.E_ARG
    assert rows(nt=n - 1) == B.E_ARG and rows(n_=-1) == B.E_ARG
    torch.cuda.synchronize()
    assert _all_nan(ar.buf), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------
# layer level
# ---------------------------------------------------------------------------------------------
COUNTED = ("mdl_mlp_head_fwd", "mdl_mlp_head_bwd", "mdl_gru_gates_fwd", "mdl_gru_gates_bwd", "mdl_loss_fwd_bwd", "mdl_loss_fwd_bwd_rows")


def _count(monkeypatch, seen):
    """wrap the entry points of the three files on the loaded library: every native call is recorded by name"""
    from matdeeplearn_amd import _lib
    L = _lib.lib()
    for n in COUNTED:
        def wrapped(*a, _n=n, _f=getattr(L, n)):
            seen.append(_n)
            return _f(*a)
        monkeypatch.setattr(L, n, wrapped)


@pytest.mark.parametrize("name,f32_out", [("ref_batch", False), ("ref_batch_f32io", True), ("ragged_widths", False)])
def test_ops_mlp_head_is_one_call_each_way_and_the_c_abi_bit_for_bit(name, f32_out, monkeypatch):
    from matdeeplearn_amd import ops
    d = dev()
    k = B.mlp_case(name)
    i, c = k["inputs"], k["spec"]
    run = _Mlp(i, c)
    layers = run.forward()
    want = run.backward(layers[:-1], det=True)
    lins = []
    for l in range(i["NL"]):
        lin = torch.nn.Linear(i["Ks"][l], i["M"][l], bias=i["b"][l] is not None).to(d)
        with torch.no_grad():
            lin.weight.copy_(i["w"][l])                              # fp32 masters that are exact in bf16: the layer's cast is exact
            if lin.bias is not None:
                lin.bias.copy_(i["b"][l])
        lins.append(lin)
    x = i["x"].to(d).to(torch.bfloat16).requires_grad_(True)
    assert ops.mlp_head_ok(x, lins, "relu")
    seen = []
    _count(monkeypatch, seen)
    with ops.deterministic(True):
        y = ops.mlp_head(x, lins, f32_out=f32_out)
        assert seen == ["mdl_mlp_head_fwd"] and y.dtype == (torch.float32 if f32_out else torch.bfloat16)
        y.backward(i["gy"].to(d).to(y.dtype))
    torch.cuda.synchronize()
    assert seen == ["mdl_mlp_head_fwd", "mdl_mlp_head_bwd"], seen
    assert torch.equal(y.detach().float().cpu(), layers[-1]) and torch.equal(x.grad.float().cpu(), want["dx"])
    for l, lin in enumerate(lins):
        assert torch.equal(lin.weight.grad.cpu(), want["dw"][l]), "dw%d" % l
        assert lin.bias is None or torch.equal(lin.bias.grad.cpu(), want["db"][l]), "db%d" % l


@pytest.mark.parametrize("name", ["v4_100_b", "s_30_b", "v4_100_f"])
def test_ops_gru_gates_is_one_call_each_way_and_the_c_abi_bit_for_bit(name, monkeypatch):
    from matdeeplearn_amd import ops
    d = dev()
    k = B.gru_case(name)
    i, c = dict(k["inputs"]), k["spec"]
    if not i["bf16"]:
        i["g_lp"], i["want_out_lp"] = None, False                    # fp32: one output serves both roles, one gradient arrives
    want, _ = _gru_launch(i, dict(c, g_lp=i["g_lp"] is not None, out_lp=i["want_out_lp"]))
    tdt = torch.bfloat16 if i["bf16"] else torch.float32
    gi, gh, h = (i[q].to(d).to(t).requires_grad_(True) for q, t in (("gi", tdt), ("gh", tdt), ("h", torch.float32)))
    assert ops.gru_gates_ok(gi, gh, h)
    seen = []
    _count(monkeypatch, seen)
    h_new, out = ops.gru_gates(gi, gh, h)
    assert seen == ["mdl_gru_gates_fwd"]
    if i["bf16"]:
        torch.autograd.backward([h_new, out], [i["g_h"].to(d), i["g_lp"].to(d).to(tdt)])
    else:
        assert out is h_new
        h_new.backward(i["g_h"].to(d))
    torch.cuda.synchronize()
    assert seen == ["mdl_gru_gates_fwd", "mdl_gru_gates_bwd"], seen
    assert torch.equal(h_new.detach().cpu(), want["h_out"]) and (not i["bf16"] or torch.equal(out.detach().float().cpu(), want["out_lp"]))
    assert torch.equal(gi.grad.float().cpu(), want["dgi"]) and torch.equal(gh.grad.float().cpu(), want["dgh"]) and torch.equal(h.grad.cpu(), want["dh"])


@pytest.mark.parametrize("name", ["rows_1024_l1", "rows_1024_mse", "n1025_l1", "n1025_mse"])
def test_ops_loss_is_one_call_and_the_c_abi_bit_for_bit(name, monkeypatch):
    from matdeeplearn_amd import ops
    d = dev()
    k = B.loss_case(name)
    i = k["inputs"]
    want = _loss_launch(i, 1)
    rows = i["n"] if i["n_total"] > i["n"] else None
    pred, y = i["p"].to(d).requires_grad_(True), i["y"].to(d)
    buf = torch.full((1 + i["n_total"] + 64,), NAN, device=d)
    seen = []
    _count(monkeypatch, seen)
    val = ops.loss("l1_loss" if i["kind"] == 0 else "mse_loss", pred, y, rows=rows, buf=buf)
    ops.backward(val)
    torch.cuda.synchronize()
    assert seen == ["mdl_loss_fwd_bwd_rows" if rows else "mdl_loss_fwd_bwd"], seen
    assert val.data_ptr() == buf.data_ptr() and _all_nan(buf[1 + i["n_total"]:]), "the value is buf[0]; nothing behind the gradient is written"
    assert torch.equal(val.detach().cpu().reshape(1), want["loss"]) and torch.equal(pred.grad.cpu(), want["grad"])
    assert torch.equal(buf[1:1 + i["n_total"]].cpu(), want["grad"])
