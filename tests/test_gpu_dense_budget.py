"""The dense layers' backward on the device against the fp64 reference, within the two measures of tests/dense_budget.py: per
row within ALLOWED times the error of the rounding model, and every fp32 element within the derived gamma_N bound.
Op level: mdl_gemm_tn_ex and mdl_dense_bwd_ex through the C ABI on every route of their dispatch — each tile shape, each
activation staging in the 4- and the 8-wave form, the scalar-load fallback, the scratch form at its edge, the deterministic shape,
strided operands at 4-byte bases — with the operands inside NaN-filled buffers (every gutter element and 70 rows behind the last
one are NaN: a read outside poisons the result) and the outputs carved out of NaN-filled arenas (what must not be written stays NaN).
Layer level: ops.linear / ops.linear_act on fp32 master weights, with the launches counted and their strides asserted.
test_dense_budget_host.py shows that these checks can fail: every mutation of the model stands at least 2 x ALLOWED over it."""
import pytest
import torch

import dense_budget as B

pytestmark = pytest.mark.gpu


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
        self.buf = torch.full((pos,), float("nan"), dtype=dtype, device=d)
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


def _operand(t, ld, off, d):
    """t [N, width] as a bf16 view with row stride ld whose first element lies `off` elements into a 16-byte aligned, NaN-filled
    buffer that also holds PAD_ROWS rows behind the last one: gutters and the rows past N are NaN"""
    N, width = t.shape
    assert ld >= width
    buf = torch.full((off + (N + B.PAD_ROWS) * ld + 8,), float("nan"), dtype=torch.bfloat16, device=d)
    assert buf.data_ptr() % 16 == 0
    v = torch.as_strided(buf, (N, width), (ld, 1), off)
    v.copy_(t)
    assert v.data_ptr() == buf.data_ptr() + 2 * off
    return v


_SCRATCH = {}


def _scratch(off, d):
    """mdl_tn_scratch_bytes() bytes full of NaN, `off` bytes past a 16-byte boundary (None: no scratch)"""
    from matdeeplearn_amd import _lib
    if off is None:
        return None
    if "buf" not in _SCRATCH:
        _SCRATCH["buf"] = torch.empty(_lib.lib().mdl_tn_scratch_bytes() // 4 + 4, device=d)
    _SCRATCH["buf"].fill_(float("nan"))
    assert off % 4 == 0 and _SCRATCH["buf"].data_ptr() % 16 == 0
    return _SCRATCH["buf"][off // 4:]


def _judge(name, route, got, c):
    """the two measures, one [budget] line, then the assertions"""
    i, s = c["inputs"], c["spec"]
    for k, v in got.items():
        assert v.shape == c["ref"][k].shape and bool(torch.isfinite(v).all()), (name, k)
    r = B.ratios(got, c["model"], c["ref"])
    f = B.bound_fraction(got, i, s["colsum"])
    print("[budget] %-20s %-30s %s   bound %s" % (name, B.route_label(route), "  ".join("%s %.4f" % kv for kv in r.items()),
                                                  "  ".join("%s %.2g (%.2f u)" % (k, v[0], v[1]) for k, v in f.items())))
    if s["act"] != 2:
        assert torch.equal(got["gm"], c["model"]["gm"]) if "gm" in got else True, "g' of a relu / plain layer is bit-equal to the model"
    if s["ints"]:
        assert torch.equal(got["dW"], c["model"]["dW"]), "integer inputs: dW is exact in any order"
        assert "db" not in got or torch.equal(got["db"], c["model"]["db"])
    over = {k: v for k, v in r.items() if not v <= B.ALLOWED[k]}
    assert not over, "%s %s: over the budget %s: %s" % (name, route, {k: B.ALLOWED[k] for k in over}, over)
    assert all(v[0] <= 1.0 for v in f.values()), "%s: over the derived bound: %s" % (name, f)


def _run_case(name):
    from matdeeplearn_amd import _lib
    d, bf16 = dev(), torch.bfloat16
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    c = B.case(name)
    i, s = c["inputs"], c["spec"]
    N, M, K, act, dense = s["N"], s["M"], s["K"], s["act"], s["kind"] == "dense"
    a = _operand(i["g"], s["lda"], s["aoff"], d)
    b = _operand(i["x"], s["ldb"], s["boff"], d)
    y = _operand(i["y"], s["ldy"], s["yoff"], d) if act else None
    w = i["w"].to(d).to(bf16).contiguous() if dense else None
    f32 = _Arena([("dW", M, K), ("db", M, 1)], torch.float32, d)
    dW, db = f32.view("dW"), f32.view("db").view(M)
    lddx = s["lddx"]
    rows = _Arena([("dX", N + B.PAD_ROWS, lddx), ("gm", N + B.PAD_ROWS, M)], bf16, d) if dense else None
    scr = _scratch(s["scratch"], d)
    flags = _lib.MDL_BF16 | (_lib.MDL_DETERMINISTIC if s["det"] else 0)
    # the route this call takes, from the pointers it passes
    scr_mod = None if scr is None else scr.data_ptr() % 16
    if dense:
        assert a.data_ptr() % 4 == 0 and b.data_ptr() % 4 == 0 and (y is None or y.data_ptr() % 4 == 0)
        route = B.dense_route(M, K, s["colsum"], act, N, scr_mod, s["det"])
    else:
        route = B.tn_route(M, K, s["colsum"], act, s["lda"], s["ldb"], a.data_ptr() % 4, b.data_ptr() % 4, N, scr_mod, s["det"])
    assert route == c["route"], (name, route)
    for off, t in ((s["aoff"], a), (s["boff"], b), (s["yoff"], y)):
        assert t is None or t.data_ptr() % 16 == (2 * off) % 16

    def launch():
        if s["prefill"]:
            dW.copy_(i["C0"]), db.copy_(i["cs0"])
        else:
            dW.zero_()
            if s["colsum"]:
                db.zero_()
        if dense:
            rows.buf.fill_(float("nan"))
            _lib.check(L.mdl_dense_bwd_ex(P(a), s["lda"], M, P(y), s["ldy"] if act else 0, act, P(b), s["ldb"], K, P(w), P(rows.view("dX")),
                                          lddx, s["xout"], P(rows.view("gm")) if s["gm"] else None, P(dW), P(db) if s["colsum"] else None,
                                          P(scr), N, flags, st()), "mdl_dense_bwd_ex")
        else:
            _lib.check(L.mdl_gemm_tn_ex(P(a), s["lda"], M, P(y), s["ldy"] if act else 0, act, P(b), s["ldb"], K, P(dW),
                                        P(db) if s["colsum"] else None, P(scr), N, flags, st()), "mdl_gemm_tn_ex")
        torch.cuda.synchronize()
        got = dict(dW=dW.cpu().clone())
        if s["colsum"]:
            got["db"] = db.cpu().clone()
        else:
            assert bool(torch.isnan(db).all()), "no column sums were asked for"
        # what the kernels must not write: the guards behind every output and the gaps in front ...
        assert bool(torch.isnan(f32.outside()).all()), "a store landed outside dW / db"
        if dense:
            assert bool(torch.isnan(rows.outside().float()).all()), "a store landed outside dX / gm"
            dx = rows.view("dX").cpu().float()
            # ... dX rows past N, the lddx - K gutter of every row ...
            assert bool(torch.isnan(dx[N:]).all()), "a dX row past N was written"
            assert bool(torch.isnan(dx[:N, K:]).all()), "the gutter of dX was written"
            got["dX"] = dx[:N, :K].contiguous()
            gm = rows.view("gm").cpu().float()
            # ... gm past N, and all of it when it is not asked for
            assert bool(torch.isnan(gm[N if s["gm"] else 0:]).all()), "gm was written past N (or without being asked for)"
            if s["gm"]:
                got["gm"] = gm[:N]
        return got

    got = launch()
    if s["det"]:                                   # one workgroup, one add per element: bit-reproducible
        again = launch()
        assert all(torch.equal(got[k], again[k]) for k in got), "the deterministic shape is not reproducible"
    _judge(name, route, got, c)


@pytest.mark.parametrize("name", list(B.TN_CASES))
def test_gemm_tn_routes_through_the_c_abi(name):
    _run_case(name)


@pytest.mark.parametrize("name", list(B.DENSE_CASES))
def test_dense_bwd_routes_through_the_c_abi(name):
    _run_case(name)


def test_the_fallback_refuses_what_it_cannot_do():
    """an activation staging or column sums on operands that only the scalar-load kernel takes: MDL_E_UNSUPP with the reason, and
    nothing written"""
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    g = torch.Generator().manual_seed(3)
    N = 100
    f32 = _Arena([("dW", 34, 160), ("db", 34, 1)], torch.float32, d)
    x = _operand(B.bfr(torch.randn(N, 160, generator=g)), 160, 0, d)
    for M, K, lda, act, cs, what in ((33, 34, 34, 1, False, "the activation staging needs even M"),
                                     (34, 34, 35, 2, False, "the activation staging needs even M"),
                                     (34, 160, 34, 0, True, "the column sums need even M"),
                                     (33, 34, 33, 0, True, "the column sums need even M")):
        a = _operand(B.bfr(torch.randn(N, M, generator=g)), lda, 0, d)
        y = _operand(B.bfr(torch.randn(N, M, generator=g)), 34, 0, d)
        assert B.tn_route(M, K, cs, act, lda, 160, a.data_ptr() % 4, x.data_ptr() % 4, N) == ("unsupp", "act" if act else "colsum")
        rc = L.mdl_gemm_tn_ex(P(a), lda, M, P(y) if act else None, 34 if act else 0, act, P(x), 160, K, P(f32.view("dW")),
                              P(f32.view("db")) if cs else None, None, N, _lib.MDL_BF16, st())
        assert rc == -2 and what in L.mdl_last_error_string().decode(), (rc, L.mdl_last_error_string())
    torch.cuda.synchronize()
    assert bool(torch.isnan(f32.buf).all())


# ---------------------------------------------------------------------------------------------
# layer level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(B.LAYER_CASES))
def test_layer_backward(name, monkeypatch):
    """ops.linear / ops.linear_act in bf16 on fp32 master weights against the fp64 layer; the launches that served the backward
    are counted, with the row stride and width each one was given (column halves and transposed chunks pass slices: ld > width,
    bases off the 16-byte grid)."""
    from matdeeplearn_amd import _lib, ops
    d, bf16 = dev(), torch.bfloat16
    c = B.layer_case(name)
    i, M, K = c["inputs"], c["M"], c["K"]
    seen = []
    L = _lib.lib()
    gemm_tn, dense_bwd = ops._gemm_tn, L.mdl_dense_bwd_ex

    def counted_tn(a, lda, m, y, ldy, act, b, ldb, k, cc, colsum, n, flags, device):
        assert n == B.LAYER_N and a.data_ptr() % 16 == 0 and (y is None) == (act == 0)
        seen.append(("tn", lda, m, ldb, k, act, colsum is not None, b.data_ptr() % 16))
        return gemm_tn(a, lda, m, y, ldy, act, b, ldb, k, cc, colsum, n, flags, device)

    def counted_dense(g, ldg, m, y, ldy, act, x, ldx, k, w, dx, lddx, xout, gm, dw, db, scratch, n, flags, stream):
        assert n == B.LAYER_N and lddx == k and xout == 0 and gm is None and (ldy == m if act else True)
        seen.append(("dense", ldg, m, ldx, k, act, db is not None))
        return dense_bwd(g, ldg, m, y, ldy, act, x, ldx, k, w, dx, lddx, xout, gm, dw, db, scratch, n, flags, stream)
    monkeypatch.setattr(ops, "_gemm_tn", counted_tn)
    monkeypatch.setattr(L, "mdl_dense_bwd_ex", counted_dense)

    x = i["x"].to(d).to(bf16).requires_grad_(c["need_dx"])
    w, b = i["w"].to(d).requires_grad_(True), i["b"].to(d).requires_grad_(True)
    out = ops.linear_act(x, w, b, c["act"]) if c["act"] else ops.linear(x, w, b)
    (out.float() * i["gout"].to(d)).sum().backward()
    torch.cuda.synchronize()
    assert seen == c["calls"], seen
    assert out.dtype == bf16 and w.grad.dtype == torch.float32 and b.grad.dtype == torch.float32
    got = dict(dW=w.grad.cpu(), db=b.grad.cpu())
    if c["need_dx"]:
        got["dX"] = x.grad.cpu().float()
    for k in got:
        assert got[k].shape == c["ref"][k].shape and bool(torch.isfinite(got[k]).all()), k
    r = {k: B.row_ratio(got[k], c["model"][k], c["ref"][k]) for k in got}
    print("[budget] %-20s %-30s %s" % (name, "%d launch(es): %s" % (len(seen), seen[0][0]), "  ".join("%s %.4f" % kv for kv in r.items())))
    over = {k: v for k, v in r.items() if not v <= B.ALLOWED[k]}
    assert not over, "%s: over the budget %s: %s" % (name, {k: B.ALLOWED[k] for k in over}, over)
