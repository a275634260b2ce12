"""BatchNorm (csrc/bn.hip) and the segmented reduce (csrc/segment.hip) on the device against the fp64 reference, within the two
measures of tests/stream_budget.py: per row within ALLOWED times the error of the rounding model, and every fp32 sum within its
derived bound.  Everything goes through the C ABI, on every route of the two dispatches, with the operands inside NaN-filled
buffers (70 NaN rows behind the last one: a read outside poisons the result) and the outputs carved out of NaN-filled arenas (what
must not be written stays NaN).  test_stream_budget_host.py shows that these checks can fail: every mutation of the model stands
at least 2 x ALLOWED over it, or breaks an equality."""
import ctypes

import pytest
import torch

import stream_budget as B

pytestmark = pytest.mark.gpu
NAN = float("nan")


def dev():
    return torch.device("cuda:0")


def _tdt(name):
    return torch.bfloat16 if name == "bf16" else torch.float32


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


def _operand(t, dtype, d, rows=None, off=0):
    """t [n, C] as the first rows of a NaN-filled buffer of `rows` (default n) + PAD_ROWS rows whose first element lies `off`
    elements past a 16-byte boundary: everything behind the data is NaN"""
    n, C = t.shape
    rows = n if rows is None else rows
    buf = torch.full((off + (rows + B.PAD_ROWS) * C + 8,), NAN, dtype=dtype, device=d)
    assert buf.data_ptr() % 16 == 0
    v = buf[off:off + rows * C].view(rows, C)
    v[:n].copy_(t)
    return v


def _all_nan(t):
    return bool(torch.isnan(t).all())


# ---------------------------------------------------------------------------------------------
# BatchNorm
# ---------------------------------------------------------------------------------------------
def _bn_launch(name, det=None, padded=True):
    """forward and backward of one case through the five entry points; padded = False runs a padded-batch case on its true rows
    alone (no n_rows_dev).  Returns the outputs on the CPU after the guard checks."""
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    c = B.bn_case(name)
    i, s = c["inputs"], c["spec"]
    tdt, dcode = _tdt(s["dtype"]), _lib.MDL_BF16 if s["dtype"] == "bf16" else _lib.MDL_F32
    N, C = i["N"], i["C"]
    cap = s["cap"] if (s["cap"] and padded) else N
    det = s["det"] if det is None else det
    route = B.bn_route(C, s["dtype"], cap, det)
    if padded and det == s["det"]:
        assert route == c["route"], (name, route)
    W = route[0]
    x, dy = _operand(i["x"], tdt, d, cap), _operand(i["dy"], tdt, d, cap)
    nd = torch.tensor([s["n_dev"]], dtype=torch.int64, device=d) if (s["n_dev"] is not None and padded) else None
    rows = _Arena([("y", cap + B.PAD_ROWS, C), ("dx", cap + B.PAD_ROWS, C)], tdt, d)
    nsum = (2 * B.R + 2) * C + (C if s["shift_row"] is not None else 0)
    assert L.mdl_bn_sums_rows() * C == (2 * B.R + 2) * C and _lib.MDL_BN_REPLICAS == B.R
    f32 = _Arena([("sums", 1, nsum), ("save", 2, C), ("rm", 1, C), ("rv", 1, C)], torch.float32, d)
    sums, save, rm, rv = f32.view("sums").view(-1), f32.view("save"), f32.view("rm").view(-1), f32.view("rv").view(-1)
    y, dx = rows.view("y"), rows.view("dx")
    for t in (x, dy, y, dx):
        assert t.data_ptr() % (W * t.element_size()) == 0
    gamma = None if i["gamma"] is None else i["gamma"].to(d)
    beta = None if i["beta"] is None else i["beta"].to(d)
    if i["rm0"] is not None:
        rm.copy_(i["rm0"]), rv.copy_(i["rv0"])
    flag = _lib.MDL_DETERMINISTIC if det else 0
    tot = slice(B.R * 2 * C, (B.R * 2 + 2) * C)

    # forward
    if s["shift_row"] is not None:
        sums[:B.R * 2 * C].copy_(i["replicas"].reshape(-1))          # the copies; the totals rows stay NaN until the kernel writes them
        sums[(2 * B.R + 2) * C:].copy_(i["x"][s["shift_row"]])        # the shift row, behind the totals rows
        dcode_apply = dcode | _lib.MDL_BN_SHIFT_ROW
    else:
        sums.zero_()
        _lib.check(L.mdl_bn_stats_n(P(x), P(sums), cap, C, P(nd), dcode | flag, st()), "mdl_bn_stats_n")
        dcode_apply = dcode
    run = i["rm0"] is not None
    _lib.check(L.mdl_bn_apply_n(P(x), P(sums), P(gamma), P(beta), P(save), P(rm) if run else None, P(rv) if run else None, P(y), cap, C,
                                B.EPS, B.MOM, P(nd), dcode_apply, st()), "mdl_bn_apply_n")
    torch.cuda.synchronize()
    got = dict(y=y.cpu().float(), s0=sums[tot].cpu()[:C].clone(), s1=sums[tot].cpu()[C:].clone(), mean=save[0].cpu(), invstd=save[1].cpu())
    if run:
        got.update(rm=rm.cpu().clone(), rv=rv.cpu().clone())
    else:
        assert _all_nan(rm) and _all_nan(rv), "running statistics were written without being asked for"
    # backward (the caller zero-fills the sums before each *_stats call)
    if s["shift_row"] is None:
        sums.zero_()
        _lib.check(L.mdl_bn_bwd_stats_n(P(dy), P(x), P(save), P(sums), cap, C, P(nd), dcode | flag, st()), "mdl_bn_bwd_stats_n")
        fn = L.mdl_bn_bwd_apply_relu_n if s["relu"] else L.mdl_bn_bwd_apply_n
        _lib.check(fn(P(dy), P(x), P(save), P(sums), P(gamma), P(dx), cap, C, P(nd), dcode, st()), "mdl_bn_bwd_apply_n")
        torch.cuda.synchronize()
        got.update(dx=dx.cpu().float(), dbeta=sums[tot].cpu()[:C].clone(), dgamma=sums[tot].cpu()[C:].clone())
    else:
        assert _all_nan(dx), "no backward ran"
    # what must not be written: guards, gaps, the rows behind the capacity; padding rows hold exact zeros
    assert _all_nan(rows.outside()) and _all_nan(f32.outside()), "a store landed outside the outputs"
    for k in ("y", "dx"):
        if k in got:
            assert _all_nan(got[k][cap:]), "%s: a row behind the last one was written" % k
            assert bool((got[k][N:cap] == 0).all()), "%s: a padding row is not exactly zero" % k
            got[k] = got[k][:N].contiguous()
    for k, v in got.items():
        assert bool(torch.isfinite(v).all()), (name, k)
    return got, route


def _bn_judge(name, got, route):
    c = B.bn_case(name)
    i, s = c["inputs"], c["spec"]
    r = B.bn_ratios(got, c["model"], c["ref"])
    f, exact = B.bn_bound_fraction(got, i)
    e_istd = float(((got["invstd"].double() - c["ref"]["invstd"]).abs() / c["ref"]["invstd"]).max())
    print("[budget] %-18s %-40s %s   bound %s   invstd rel err %.2g" % (
        name, B.bn_label(route), "  ".join("%s %.3f" % kv for kv in r.items()), "  ".join("%s %.2g" % kv for kv in f.items()), e_istd))
    if s["kind"] == "ints":
        assert torch.equal(got["s0"].double(), exact["s0"]) and torch.equal(got["s1"].double(), exact["s1"]), "integer inputs: the totals are exact"
        assert torch.equal(got["dbeta"], c["model"]["dbeta"]), "integer inputs: dbeta is exact"
    if s["relu"]:
        assert bool((got["dx"][i["x"] <= 0] == 0).all()), "dx is exactly zero where the ReLU output is"
    if i["N"] == 1:
        # one row: var = 0, mean = the row, y = beta up to the rounding of beta - mean * scale in fp32 and of y to bf16, dx = 0
        big = (i["x"][0] * i["gamma"]).abs() * B.EPS ** -0.5
        assert bool(((got["y"][0] - i["beta"]).abs() <= 4 * B.U * big + 2.0 ** -8 * i["beta"].abs()).all()), "one row: y = beta"
        assert torch.equal(got["mean"], i["x"][0]) and float(got["dx"].abs().max()) == 0.0
        assert bool(((got["rv"] - ((1 - B.MOM) * i["rv0"])).abs() <= 1e-6).all()), "one row: running_var takes the biased variance, 0"
    over = {k: v for k, v in r.items() if not v <= B.ALLOWED[k]}
    assert not over, "%s: over the budget %s: %s" % (name, {k: B.ALLOWED[k] for k in over}, over)
    assert all(v <= 1.0 for v in f.values()), "%s: over the derived bound: %s" % (name, f)


@pytest.mark.parametrize("name", list(B.BN_CASES))
def test_batchnorm_routes_through_the_c_abi(name):
    s = B.BN_CASES[name]
    got, route = _bn_launch(name)
    if s["det"]:                                                     # one reduce block, one add per sum: bit-reproducible
        again, _ = _bn_launch(name)
        assert all(torch.equal(got[k], again[k]) for k in got), "MDL_DETERMINISTIC is not reproducible"
    _bn_judge(name, got, route)
    if s["n_dev"] is not None:
        # under MDL_DETERMINISTIC the reduce grid is 1 whatever the capacity: the padded call IS the unpadded one, bit for bit
        a, _ = _bn_launch(name, det=True)
        b, _ = _bn_launch(name, det=True, padded=False)
        assert all(torch.equal(a[k], b[k]) for k in a), [k for k in a if not torch.equal(a[k], b[k])]


def test_batchnorm_relu_backward_refuses_fp32():
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    N, C = 130, 64
    x, dy = torch.randn(N, C, device=d), torch.randn(N, C, device=d)
    f32 = _Arena([("dx", N, C), ("sums", 1, (2 * B.R + 2) * C), ("save", 2, C)], torch.float32, d)
    rc = L.mdl_bn_bwd_apply_relu_n(P(dy), P(x), P(f32.view("save")), P(f32.view("sums")), None, P(f32.view("dx")), N, C, None, _lib.MDL_F32, st())
    torch.cuda.synchronize()
    assert rc == -2 and "bf16 only" in L.mdl_last_error_string().decode(), (rc, L.mdl_last_error_string())
    assert _all_nan(f32.buf), "a refused call wrote something"


def test_batchnorm_refuses_bad_pointers_before_any_launch():
    """a null or misaligned y / dy / dx and a null sums / save: MDL_E_ARG, a message that names the tensor, nothing written"""
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    N, C = 130, 64
    for dtype, code in ((torch.bfloat16, _lib.MDL_BF16), (torch.float32, _lib.MDL_F32)):
        x, dy = torch.randn(N, C, device=d).to(dtype), torch.randn(N, C, device=d).to(dtype)
        rows = _Arena([("y", N, C), ("dx", N, C)], dtype, d)
        f32 = _Arena([("sums", 1, (2 * B.R + 2) * C), ("save", 2, C)], torch.float32, d)
        y, dx, sums, save = rows.view("y"), rows.view("dx"), f32.view("sums"), f32.view("save")
        off = lambda t, nbytes: ctypes.c_void_p(t.data_ptr() + nbytes)            # inside the tensor's own allocation
        half = 8 if dtype == torch.bfloat16 else 4                              # aligned to the element, not to the 16-byte vector
        apply = lambda xx, ss, sv, yy: L.mdl_bn_apply_n(xx, ss, None, None, sv, None, None, yy, N, C, B.EPS, B.MOM, None, code, st())
        bstats = lambda dd, xx, sv, ss: L.mdl_bn_bwd_stats_n(dd, xx, sv, ss, N, C, None, code, st())
        bapply = lambda fn: (lambda dd, xx, sv, ss, dxx: fn(dd, xx, sv, ss, None, dxx, N, C, None, code, st()))
        calls = [("x", lambda: L.mdl_bn_stats_n(None, P(sums), N, C, None, code, st())),
                 ("sums", lambda: L.mdl_bn_stats_n(P(x), None, N, C, None, code, st())),
                 ("x", lambda: L.mdl_bn_stats_n(off(x, half), P(sums), N, C, None, code, st())),
                 ("y", lambda: apply(P(x), P(sums), P(save), None)), ("y", lambda: apply(P(x), P(sums), P(save), off(y, half))),
                 ("sums", lambda: apply(P(x), None, P(save), P(y))), ("save", lambda: apply(P(x), P(sums), None, P(y))),
                 ("dy", lambda: bstats(None, P(x), P(save), P(sums))), ("dy", lambda: bstats(off(dy, half), P(x), P(save), P(sums))),
                 ("save", lambda: bstats(P(dy), P(x), None, P(sums))), ("sums", lambda: bstats(P(dy), P(x), P(save), None))]
        for fn in (L.mdl_bn_bwd_apply_n,) + ((L.mdl_bn_bwd_apply_relu_n,) if dtype == torch.bfloat16 else ()):
            ba = bapply(fn)
            calls += [("dy", lambda ba=ba: ba(None, P(x), P(save), P(sums), P(dx))), ("dy", lambda ba=ba: ba(off(dy, half), P(x), P(save), P(sums), P(dx))),
                      ("x", lambda ba=ba: ba(P(dy), off(x, half), P(save), P(sums), P(dx))),
                      ("dx", lambda ba=ba: ba(P(dy), P(x), P(save), P(sums), None)), ("dx", lambda ba=ba: ba(P(dy), P(x), P(save), P(sums), off(dx, half))),
                      ("sums", lambda ba=ba: ba(P(dy), P(x), P(save), None, P(dx))), ("save", lambda ba=ba: ba(P(dy), P(x), None, P(sums), P(dx)))]
        for what, call in calls:
            rc = call()
            msg = L.mdl_last_error_string().decode()
            assert rc == -1 and (": %s is " % what) in msg, (what, rc, msg)
        torch.cuda.synchronize()
        assert _all_nan(rows.buf) and _all_nan(f32.buf), "a refused call wrote something"


# ---------------------------------------------------------------------------------------------
# segment reduce
# ---------------------------------------------------------------------------------------------
def _seg_run(name):
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    c = B.seg_case(name)
    i, s = c["inputs"], c["spec"]
    tdt, dcode = _tdt(s["dtype"]), _lib.MDL_BF16 if s["dtype"] == "bf16" else _lib.MDL_F32
    N, E, C, red = i["N"], i["E"], i["C"], _lib.REDUCE[i["reduce"]]
    src = _operand(i["src"], tdt, d, off=s["src_off"])
    go = _operand(i["go"], tdt, d)
    add = None if i["addend"] is None else _operand(i["addend"], tdt, d)
    perm = None if i["perm"] is None else i["perm"].to(torch.int32).to(d)
    cnt = i["rowptr"][1:] - i["rowptr"][:-1]
    seg = torch.repeat_interleave(torch.arange(N), cnt).to(torch.int32).to(d)
    # the row pointer from the sorted segment index, on the device: inside a NaN-free int arena of its own
    rp_buf = torch.full((N + 1 + 64,), -7, dtype=torch.int32, device=d)
    _lib.check(L.mdl_csr_rowptr(P(seg), E, N, P(rp_buf), st()), "mdl_csr_rowptr")
    assert torch.equal(rp_buf[:N + 1].cpu().long(), i["rowptr"]) and bool((rp_buf[N + 1:] == -7).all()), "mdl_csr_rowptr"
    rowptr = rp_buf[:N + 1]
    outs = _Arena([("out", N + B.PAD_ROWS, C), ("gsrc", E + B.PAD_ROWS, C)], tdt, d)
    out, gsrc = outs.view("out"), outs.view("gsrc")
    am = torch.full((N * C + 128,), -7, dtype=torch.int32, device=d)
    mod = lambda t: t.data_ptr() % 16
    routes = dict(fwd=B.seg_route("fwd", i["reduce"], s["dtype"], N, E, C, (mod(src), mod(out))),
                  bwd=B.seg_route("bwd", i["reduce"], s["dtype"], N, E, C, (mod(go), mod(gsrc))))
    if add is not None:
        routes["bwd_add"] = B.seg_route("bwd_add", i["reduce"], s["dtype"], N, E, C, (mod(go), mod(gsrc), mod(add)))
    assert routes == c["routes"], (name, routes)
    is_max = i["reduce"] == "max"

    def forward():
        outs.buf.fill_(NAN)
        _lib.check(L.mdl_segment_reduce_fwd(P(src), P(rowptr), P(perm), P(out), P(am) if is_max else None, N, C, red, dcode, st()), "fwd")
        torch.cuda.synchronize()
        o = out.cpu().float()
        assert _all_nan(outs.outside()) and _all_nan(o[N:]) and _all_nan(gsrc), "the forward wrote outside out"
        return o[:N].contiguous()

    got = dict(out=forward())
    assert torch.equal(forward(), got["out"]), "the forward is atomic-free: two runs are bit-equal"
    assert bool(torch.isfinite(got["out"]).all())

    def backward(addend):
        gsrc.fill_(NAN)
        if is_max:
            gsrc[:E].zero_()                                         # max writes the argmax rows only: zero-filled by the caller, as ops does
        if addend is None:
            _lib.check(L.mdl_segment_reduce_bwd(P(go), P(rowptr), P(seg), P(perm), P(am) if is_max else None, P(gsrc), N, E, C, red, dcode, st()), "bwd")
        else:
            _lib.check(L.mdl_segment_reduce_bwd_add(P(go), P(rowptr), P(seg), P(perm), P(addend), P(gsrc), N, E, C, red, dcode, st()), "bwd_add")
        torch.cuda.synchronize()
        g = gsrc.cpu().float()
        assert _all_nan(outs.outside()) and _all_nan(g[E:]), "the backward wrote outside grad_src"
        assert bool(torch.isfinite(g[:E]).all())
        return g[:E].contiguous()

    got["gsrc"] = backward(None)
    if add is not None:
        got["gsrc_add"] = backward(add)
    label = "%s | %s%s" % (B.seg_label(routes["fwd"]), B.seg_label(routes["bwd"]), " | +add" if add is not None else "")
    if is_max:
        assert bool((am[N * C:] == -7).all()), "argmax was written past N * C"
        assert torch.equal(got["out"], c["model"]["out"]) and torch.equal(got["out"].double(), c["ref"]["out"]), "max is exact"
        assert torch.equal(am[:N * C].view(N, C).cpu(), c["model"]["argmax"]), "argmax is the first maximum (-1: empty)"
        assert torch.equal(got["gsrc"], c["model"]["gsrc"]), "the gradient goes to the argmax row"
        print("[budget] %-28s %-34s exact" % (name, label))
        return
    r = B.seg_ratios(got, c["model"], c["ref"])
    f = B.seg_bound_fraction(got["out"], i)
    print("[budget] %-28s %-34s %s   bound out %.2g" % (name, label, "  ".join("%s %.3f" % kv for kv in r.items()), f))
    if s["ints"]:
        assert all(torch.equal(got[k], c["model"][k]) for k in got), "integer inputs: exact in any order"
    if i["reduce"] == "sum":
        assert torch.equal(got["gsrc"], c["model"]["gsrc"]), "the backward of a sum is a copy"
    over = {k: v for k, v in r.items() if not v <= B.ALLOWED[k]}
    assert not over, "%s: over the budget %s: %s" % (name, {k: B.ALLOWED[k] for k in over}, over)
    assert f <= 1.0, "%s: over the derived bound: %s" % (name, f)


@pytest.mark.parametrize("name", list(B.SEG_CASES))
def test_segment_reduce_routes_through_the_c_abi(name):
    _seg_run(name)


def test_segment_bwd_add_refuses_rows_without_a_vector_width():
    from matdeeplearn_amd import _lib
    d = dev()
    L, P, st = _lib.lib(), _lib.ptr, _lib.stream
    N, E, C = 5, 20, 50
    assert B.seg_route("bwd_add", "sum", "bf16", N, E, C, (0, 0, 0)) == ("unsupp",) == B.seg_route("bwd_add", "mean", "f32", N, E, C, (0, 0, 0))
    rowptr = torch.arange(0, E + 1, 4, dtype=torch.int32, device=d)
    seg = torch.repeat_interleave(torch.arange(N), 4).to(torch.int32).to(d)
    for dtype, code in ((torch.bfloat16, _lib.MDL_BF16), (torch.float32, _lib.MDL_F32)):
        go, add = torch.randn(N, C, device=d).to(dtype), torch.randn(E, C, device=d).to(dtype)
        outs = _Arena([("gsrc", E, C)], dtype, d)
        rc = L.mdl_segment_reduce_bwd_add(P(go), P(rowptr), P(seg), None, P(add), P(outs.view("gsrc")), N, E, C, _lib.MDL_SUM, code, st())
        torch.cuda.synchronize()
        assert rc == -2 and "vector multiple" in L.mdl_last_error_string().decode(), (rc, L.mdl_last_error_string())
        assert _all_nan(outs.buf), "a refused call wrote something"
