"""Error budget of the dense layers' backward against an fp64 reference (helper module of test_dense_budget_host.py and
test_gpu_dense_budget.py; no test lives here).  It follows tests/nnconv_budget.py: the yardstick is a ROUNDING MODEL, the same
arithmetic in plain fp32 torch on the CPU, rounded to bf16 exactly where the kernel rounds; a kernel output may stand
ALLOWED[tensor] times the model's own distance from fp64, per row (row_ratio), and a structural bug stands far over it (MUTATIONS).

One kernel body serves every case: gemm_tn_stream_kernel (csrc/gemm_tn_stream.inc), instantiated by
  mdl_gemm_tn_ex    (csrc/gemm_tn.hip)    C[M, K] += (A .* act'(Y))^T B,  colsum[M] += column sums     TN_CASES
  mdl_dense_bwd_ex  (csrc/dense_bwd.hip)  the same with dX = (A .* act'(Y)) W .* act_in'(B) and g'      DENSE_CASES
and reached from every Linear through ops.linear / ops.linear_act                                        LAYER_CASES
In the terms of a layer y = act(x W^T + b):  A = g (gradient w.r.t. y), B = x, C = dW, colsum = db, GM = g' = g .* act'(y).

Two measures:
  tight    row_ratio(got, model, ref64) <= ALLOWED[tensor]; rows are output units for dW, one row for db, data rows for dX / gm.
           For act = 0 / 1 both operands of dW = g'^T x are exact bf16 values: the model's error IS fp32 summation noise, and the
           ratio compares the kernel's summation order (16-row MFMA steps, one accumulator per workgroup, the workgroups added
           with atomics or by tn_reduce_kernel) with torch's.  For act = 2 the rounding of g' to bf16 dominates both sides.
  derived  |got - exact| <= N 2^-24 sum_n |g'_nm| |x_nk| for every element of the fp32 outputs, `exact` the fp64 product of the
           operands the kernel multiplies (g' as the model rounds it).  bf16 x bf16 is exact in fp32, so an fp32 sum of N such
           products in ANY order obeys the gamma_N bound; nothing in it is measured.  db: the same with x = 1.  A prefilled
           output is one more term.  bound_fraction() reports the largest |got - exact| in units of that bound.

The table of measured ratios per case and route stands in front of ALLOWED below.
"""
import functools

import torch

from cgconv_budget import bfr, fmt, row_ratio, row_rms  # noqa: F401  (re-exported for the tests)

LN2 = 0.6931471805599453
TENSORS = ("dW", "db", "dX", "gm")
PAD_ROWS = 70                                    # NaN rows behind every operand and every row-shaped output (more than one tile)
GUARD = 256                                      # bytes behind every output in the arenas of the GPU test
U = 2.0 ** -24                                   # unit roundoff of fp32

# Permitted row_ratio per tensor: twice the largest value measured on the MI355X over every case of test_gpu_dense_budget.py and
# two runs, rounded up to one decimal, never below 2 and never above 5.  The factor 2 covers what kernel and model draw
# differently: the summation order, which atomics make different from run to run wherever more than one workgroup adds.
# Measured on the MI355X (one run; `largest` is over two): row_ratio per case against the rounding model, and `bound`, the largest
# |got - exact| as a fraction of the derived bound N 2^-24 sum|g'||x| (in units of 2^-24 sum|g'||x| it was 0.3 - 1.9 everywhere).
#   case                route                           ratios
#   t11_k30             stream <1,1> NW4 grid 1         dW 0.000 db 0.000   bound dW 0 db 0
#   t12_k32             stream <1,2> NW4 grid 1         dW 1.197 db 0.000   bound dW 0.024 db 0
#   t14_k94             stream <1,4> NW4 grid 1         dW 1.000 db 1.000   bound dW 0.017 db 0.0049
#   t15_k128            stream <1,5> NW8 grid 1         dW 0.938 db 0.000   bound dW 0.018 db 0
#   t21                 stream <2,1> NW4 grid 2         dW 1.061 db 0.000   bound dW 0.015 db 0
#   t22                 stream <2,2> NW4 grid 2         dW 1.000 db 1.000   bound dW 0.0099 db 0.0006
#   t24_k96             stream <2,4> NW4 grid 4         dW 1.024 db 0.000   bound dW 0.0038 db 0
#   t25_k158            stream <2,5> NW8 grid 4         dW 1.192 db 1.000   bound dW 0.0045 db 0.00045
#   t41_m66             stream <4,1> NW4 grid 1         dW 1.000 db 1.000   bound dW 0.042 db 0
#   t42                 stream <4,2> NW4 grid 2         dW 1.393   bound dW 0.016
#   t44                 stream <4,4> NW4 grid 2         dW 1.162   bound dW 0.013
#   t45_k160            stream <4,5> NW8 grid 1         dW 1.000   bound dW 0.021
#   t51                 stream <5,1> NW8 grid 1         dW 1.267 db 0.000   bound dW 0.019 db 0
#   t52                 stream <5,2> NW8 grid 1         dW 0.000 db 0.000   bound dW 0 db 0
#   t54                 stream <5,4> NW8 grid 4         dW 1.000 db 1.000   bound dW 0.0055 db 0.00094
#   t55                 stream <5,5> NW8 grid 2         dW 1.067 db 1.000   bound dW 0.029 db 0.0014
#   det200              stream <2,2> NW4 grid 1         dW 1.631 db 1.000   bound dW 0.0045 db 0.0011
#   prefetch            stream <2,2> NW4 grid 256       dW 0.000 db 0.000   bound dW 0 db 0
#   cap512              stream <1,1> NW4 grid 512       dW 0.000 db 0.000   bound dW 0 db 0
#   part_off            stream <2,2> NW4 grid 31        dW 1.252 db 1.116   bound dW 0.00018 db 2.6e-05
#   part_on             stream <2,2> NW4 grid 32 part   dW 0.984 db 0.851   bound dW 0.00015 db 2e-05
#   part_on_bumped      stream <4,4> NW4 grid 33 part   dW 1.144 db 0.974   bound dW 0.00017 db 2.1e-05
#   scratch_misaligned  stream <2,2> NW4 grid 32        dW 1.289 db 0.846   bound dW 0.00016 db 2e-05
#   prefill             stream <2,2> NW4 grid 4         dW 1.067 db 1.000   bound dW 0.0025 db 0.00047
#   strided             stream <1,1> NW4 grid 2         dW 1.211 db 0.000   bound dW 0.013 db 0
#   strided_wide        stream <5,4> NW8 grid 4         dW 1.000 db 1.000   bound dW 0.0052 db 0.001
#   fb11_base2          fallback <1,1> grid 2           dW 1.254   bound dW 0.0023
#   fb21_odd_m          fallback <2,1> grid 2           dW 1.154   bound dW 0.003
#   fb31_odd_k          fallback <3,1> grid 2           dW 1.351   bound dW 0.0072
#   fb41_odd_lda        fallback <4,1> grid 2           dW 1.124   bound dW 0.0046
#   fb12_k200           fallback <1,2> grid 2           dW 0.985   bound dW 0.0045
#   fb22_k200           fallback <2,2> grid 1           dW 0.946   bound dW 0.018
#   fb32_k256           fallback <3,2> grid 2           dW 1.166   bound dW 0.0046
#   fb42_k256           fallback <4,2> grid 3           dW 0.957   bound dW 0.0032
#   fb51_m130_odd_lda   fallback <5,1> grid 2           dW 1.193   bound dW 0.0033
#   d22                 dx <2,2> NW8 grid 1             dW 0.000 db 0.000 dX 1.000   bound dW 0 db 0
#   d24_k66             dx <2,4> NW4 grid 1             dW 1.123 db 0.000 dX 1.000 gm 0.000   bound dW 0.031 db 0
#   d25_k158            dx <2,5> NW8 grid 1             dW 1.000 db 1.000 dX 1.000   bound dW 0.045 db 0
#   d42_m66             dx <4,2> NW4 grid 1             dW 1.000 dX 1.000 gm 1.000   bound dW 0.019
#   d44_k94             dx <4,4> NW4 grid 2             dW 1.097 db 0.000 dX 1.000   bound dW 0.025 db 0
#   d44_nodb_k66        dx <4,4> NW8 grid 2             dW 1.027 dX 1.000   bound dW 0.012
#   d45_k160            dx <4,5> NW8 grid 2             dW 1.123 dX 1.000   bound dW 0.015
#   d52_m160            dx <5,2> NW8 grid 4             dW 1.000 db 1.000 dX 1.000   bound dW 0.0058 db 0.0014
#   d54                 dx <5,4> NW8 grid 2             dW 1.068 db 0.000 dX 1.000 gm 0.000   bound dW 0.017 db 0
#   d55                 dx <5,5> NW8 grid 4             dW 1.127 db 1.000 dX 1.000 gm 0.000   bound dW 0.005 db 0.0005
#   d_strided           dx <4,4> NW4 grid 2             dW 1.000 db 1.000 dX 1.000 gm 1.000   bound dW 0.011 db 0.0011
#   d_strided_relu      dx <2,2> NW4 grid 1             dW 1.374 db 0.000 dX 1.000   bound dW 0.031 db 0
#   d_det200            dx <2,2> NW4 grid 1             dW 1.400 db 1.000 dX 1.000   bound dW 0.0036 db 0.00023
#   d_part_off          dx <2,2> NW8 grid 31            dW 1.118 db 1.510 dX 1.000   bound dW 0.00016 db 6.3e-05
#   d_part_on           dx <2,2> NW4 grid 32 part       dW 1.000 db 1.000 dX 1.000 gm 1.000   bound dW 0.00026 db 2.6e-05
#   d_prefetch          dx <2,2> NW4 grid 256           dW 0.000 db 0.000 dX 1.000   bound dW 0 db 0
#   d_prefill           dx <2,2> NW8 grid 4             dW 1.173 db 1.000 dX 1.000   bound dW 0.003 db 0.00016
#   dense_relu          1 launch(es): dense             dW 1.100 db 0.000 dX 1.000
#   dense_ssp           1 launch(es): dense             dW 1.000 db 1.000 dX 1.000
#   tn_act              1 launch(es): tn                dW 0.963 db 0.000
#   odd_m               1 launch(es): tn                dW 0.673 db 1.000 dX 1.000
#   k258                2 launch(es): tn                dW 0.812 db 1.000 dX 1.000
#   k300                2 launch(es): tn                dW 0.832 db 1.000 dX 1.000
#   k320                2 launch(es): tn                dW 0.823 db 0.123 dX 1.000
#   m162                2 launch(es): tn                dW 1.027 db 1.000 dX 1.000
#   m450                3 launch(es): tn                dW 0.995 db 1.004 dX 1.000
# largest: dW 1.6315 (det200), db 1.5098 (d_part_off), dX 1.0000, gm 1.0000; of the derived bound: dW 0.045 (d25_k158), db 0.0049.
# 0.000: model and kernel both exact (one row; integer inputs; db, whose sums of a few hundred bf16 values are exact in fp32).
# 1.000: the rounding of g' (act = 2) or of dX to bf16 dominates both sides.  No ratio came near 2.5: no rounding point is missing
# from the model.  One launcher bug was found by reading the dispatch for the mirror, not by a ratio: the scalar-load fallback
# served 128 < M <= 160 with its 4-tile instantiation and left rows 128 .. M - 1 of C unwritten (fb51_m130_odd_lda pins the fix).
ALLOWED = {"dW": 3.3, "db": 3.1, "dX": 2.0, "gm": 2.0}


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# the dispatch of the two launchers, restated: the kernel choice is made in C and is not observable from Python
# ---------------------------------------------------------------------------------------------
def _tiles(M, K, extra):
    """(mt, nt) of csrc/gemm_tn.hip:123-125 and csrc/dense_bwd.hip:42-44: 32-wide tiles, the bias sums in padding column K of the B
    tile, three tiles served by the four-tile instantiation"""
    mt, nt = cdiv(M, 32), cdiv(K + (1 if extra else 0), 32)
    return (4 if mt == 3 else mt), (4 if nt == 3 else nt)


def _grid(N, mt, nt, det):
    """csrc/gemm_tn.hip:133-135, csrc/dense_bwd.hip:45-47: one workgroup per 64-row tile up to the cap"""
    cap = 1 if det else (512 if N >= (1 << 20) and mt * nt < 25 else 256)
    return min(cdiv(N, 64), cap)


def tn_route(M, K, colsum, act, lda, ldb, a_mod4, b_mod4, N, scratch_mod16=None, det=False):
    """The kernel mdl_gemm_tn_ex launches (csrc/gemm_tn.hip), from what the caller passes: a_mod4 / b_mod4 = the A / B base address
    modulo 4, scratch_mod16 = the scratch address modulo 16 (None: no scratch), det = the MDL_DETERMINISTIC flag.
      ("stream", mt, nt, NW, grid, part)  gemm_tn_stream_kernel<mt, nt, act, false, NW>: even M, K, lda, ldb, dword-aligned bases and
                                          at most 5 column tiles (lines 126-128); NW = 8 where a side has 5 tiles (line 17);
                                          part = the scratch form + tn_reduce_kernel (line 138: 16-byte aligned scratch, not
                                          deterministic, at least 32 workgroups)
      ("fallback", mt, ntw, grid)         gemm_tn_kernel<mt, ntw> (lines 160-172): 128 rows per step, at most 512 workgroups; mt = 5
                                          (128 < M <= 160) is two launches, <4, ntw> and <1, ntw> on the columns from 128
      ("unsupp", what)                    the fallback takes neither an activation staging nor column sums (lines 158-159)"""
    assert 1 <= M <= 160 and 1 <= K <= 256 and (M <= 128 or (K <= 160 and M % 2 == 0 and K % 2 == 0)), "line 117"
    mt, nt = _tiles(M, K, colsum)
    if M % 2 == 0 and K % 2 == 0 and lda % 2 == 0 and ldb % 2 == 0 and nt <= 5 and a_mod4 == 0 and b_mod4 == 0:
        grid = _grid(N, mt, nt, det)
        part = scratch_mod16 == 0 and not det and grid >= 32
        return ("stream", mt, nt, 8 if mt > 4 or nt > 4 else 4, grid, part)
    if act != 0:
        return ("unsupp", "act")
    if colsum:
        return ("unsupp", "colsum")
    return ("fallback", cdiv(M, 32), (cdiv(K, 32) + 3) // 4, 1 if det else min(cdiv(N, 128), 512))


def dense_route(M, K, db, act, N, scratch_mod16=None, det=False):
    """("dx", mt, nt, NW, grid, part): the instantiation gemm_tn_stream_kernel<mt, nt, act, true, NW> of mdl_dense_bwd_ex
    (csrc/dense_bwd.hip): 8 waves without an activation staging and for every shape with a 5-tile side, else 4 (lines 59-68)"""
    assert 34 <= M <= 160 and 34 <= K <= (158 if db else 160) and M % 2 == 0 and K % 2 == 0, "line 32"
    mt, nt = _tiles(M, K, db)
    grid = _grid(N, mt, nt, det)
    return ("dx", mt, nt, 8 if act == 0 or mt > 4 or nt > 4 else 4, grid, scratch_mod16 == 0 and not det and grid >= 32)


def route_label(route):
    if route[0] == "fallback":
        return "fallback <%d,%d> grid %d" % route[1:]
    return "%s <%d,%d> NW%d grid %d%s" % (route[0], route[1], route[2], route[3], route[4], " part" if route[5] else "")


# ---------------------------------------------------------------------------------------------
# inputs, fp64 reference, rounding model
# ---------------------------------------------------------------------------------------------
def make_inputs(N, M, K, act, xout, seed, ints=False, prefill=False, dx=False):
    """fp32 tensors that are exact in bf16: g [N, M] ~ N(0, 1); y [N, M] = relu(pre) (exact zeros) or ssp(pre); x [N, K] plain,
    relu or ssp according to xout; w [M, K] ~ N(0, 1 / M).  One more row of each (`*_pad`) and one more column of g (`a_gutter`)
    stand for what lies behind the arrays: only the mutations read them.  prefill: small integers that C / colsum hold on entry.
    ints: g, x in {-3 .. 3} (N(0, 1) rounded to the integer grid): every partial sum of up to 2^20 + 1 products is an integer
    below 2^24, so the fp32 result is EXACT in any order — the model has no error, and any error of the kernel is infinitely over.
    The cases with N >= 16453 take it: there torch's blocked CPU sum is several times more accurate than ANY order that adds 256
    workgroup sums one after the other (the emulated kernel order stands 3.4 - 4.9 x over it at N = 16453), so a row_ratio against
    it would measure torch's summation, not the kernel's.  What those cases are for — every row summed exactly once by the tile
    loop, the prefetch and the 512-workgroup grid — is checked by equality instead."""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    ssp = lambda v: torch.nn.functional.softplus(v) - LN2
    fn = {0: lambda v: v, 1: torch.relu, 2: ssp}
    if ints:
        assert act in (0, 1) and xout in (0, 1), "a softplus factor is no integer"
        g, x = rnd(N + 1, M).round().clamp(-3, 3), fn[xout](rnd(N + 1, K).round().clamp(-3, 3))
    else:
        g, x = bfr(rnd(N + 1, M)), bfr(fn[xout](rnd(N + 1, K) * (2.0 if xout else 1.0)))
    y = bfr(fn[act](rnd(N + 1, M) * 2.0)) if act else None
    i = dict(N=N, M=M, K=K, act=act, xout=xout, g=g[:N], x=x[:N], y=None if y is None else y[:N], g_pad=g[N:], x_pad=x[N:],
             y_pad=None if y is None else y[N:], a_gutter=bfr(rnd(N)), w=bfr(rnd(M, K) / M ** 0.5) if dx else None)
    i["C0"] = torch.randint(-4, 5, (M, K), generator=gen).float() if prefill else None
    i["cs0"] = torch.randint(-4, 5, (M,), generator=gen).float() if prefill else None
    return i


def dact(code, v, dtype):
    """act'(.) as a function of the activation's OUTPUT: relu v > 0, shifted softplus 1 - exp(-(v + ln 2))"""
    v = v.to(dtype)
    if code == 1:
        return (v > 0).to(dtype)
    if code == 2:
        return 1.0 - torch.exp(-(v + LN2))
    return torch.ones_like(v)


def n_tiles(N):
    return cdiv(N, 64)


def compute(i, dtype=torch.float32, rounded=True, colsum=True, mutation=None):
    """dict(dW, db, dX, gm) of one case in `dtype`; rounded: round to bf16 where the kernel does; mutation: a key of MUTATIONS"""
    N, M, K, act, xout = i["N"], i["M"], i["K"], i["act"], i["xout"]
    r = bfr if rounded else (lambda t: t)
    g, x = i["g"].to(dtype), i["x"].to(dtype)

    def gprime(g, y):
        if act == 0:
            return g
        if act == 1:
            return g * ((y >= 0) if mutation == "mask_ge" else (y > 0)).to(dtype)
        gp = r(g * dact(2, y, dtype))
        return r(gp * dact(2, y, dtype)) if mutation == "staged_twice" else gp
    gp = gprime(g, i["y"])
    keep = torch.ones(N, 1, dtype=dtype)
    if mutation == "drop_last_row":
        keep[N - 1] = 0
    if mutation == "drop_tile":
        t = (n_tiles(N) - 1) // 2
        keep[64 * t:64 * t + 64] = 0
    a, b = gp * keep, x
    if mutation == "row_past_n":
        a, b = torch.cat([a, gprime(i["g_pad"].to(dtype), i["y_pad"])]), torch.cat([b, i["x_pad"].to(dtype)])
    if mutation == "gutter_column":
        a = a.clone()
        a[:N, M - 1] = i["a_gutter"].to(dtype)
    dW, db = a.t() @ b, a.sum(0)
    if mutation == "bias_into_dw":
        dW[:, K - 1] += db
    if i["C0"] is not None:
        dW, db = dW + i["C0"].to(dtype), db + i["cs0"].to(dtype)
    out = dict(dW=dW, gm=gp)
    if colsum:
        out["db"] = db
    if i["w"] is not None:
        f = dact(xout, x, dtype)
        if mutation == "xout_skipped_second_block":
            f[(torch.arange(N) % 64) >= 32] = 1.0
        out["dX"] = r((gp @ i["w"].to(dtype)) * f)
    return out


def reference64(i, colsum=True):
    """g' = g .* act'(y), dW = g'^T x, db = sum g', dX = (g' W) .* act_in'(x) in fp64, nothing rounded"""
    return compute(i, torch.float64, rounded=False, colsum=colsum)


def model(i, colsum=True, mutation=None):
    """The kernel in plain fp32 torch, rounded where it rounds (csrc/gemm_tn_stream.inc):
      g'   relu: the mask y > 0 on the bf16 g, exact (line 141); shifted softplus: g * (1 - exp(-(y + ln 2))) in fp32, rounded to
           bf16 once (lines 143-145) — the value that enters all three products and leaves as gm (lines 170, 179)
      dW   fp32 sums of exact products of g' and x (MFMA accumulators, then atomics / tn_reduce_kernel)
      db   the same product with a column of ones (lines 189, 198)
      dX   fp32 sums of g' W, the act_in'(x) factor on the fp32 value, ONE rounding to bf16 on store (lines 260-266)"""
    return compute(i, torch.float32, rounded=True, colsum=colsum, mutation=mutation)


def exact_products(i, colsum=True):
    """(exact, mag) per fp32 tensor for the derived bound: the fp64 product of the operands the kernel multiplies (g' as the model
    rounds it) and sum_n |g'_nm| |x_nk| (+ |prefill|)"""
    gp, x = model(i)["gm"].double(), i["x"].double()
    ex, mag = {"dW": gp.t() @ x, "db": gp.sum(0)}, {"dW": gp.abs().t() @ x.abs(), "db": gp.abs().sum(0)}
    if i["C0"] is not None:
        ex = {"dW": ex["dW"] + i["C0"].double(), "db": ex["db"] + i["cs0"].double()}
        mag = {"dW": mag["dW"] + i["C0"].abs().double(), "db": mag["db"] + i["cs0"].abs().double()}
    return {k: (ex[k], mag[k]) for k in (("dW", "db") if colsum else ("dW",))}


def bound_fraction(got, i, colsum=True):
    """{tensor: (largest |got - exact| / (terms 2^-24 sum|.||.|), the same in units of 2^-24 sum|.||.|)}; terms = N (+ 1 prefilled)"""
    terms = i["N"] + (1 if i["C0"] is not None else 0)
    out = {}
    for k, (ex, mag) in exact_products(i, colsum).items():
        err = (got[k].double() - ex).abs()
        assert bool((err[mag == 0] == 0).all()), "%s: a sum of zeros is not zero" % k
        units = float((err / mag.clamp(min=1e-300) / U)[mag > 0].max()) if bool((mag > 0).any()) else 0.0
        out[k] = (units / terms, units)
    return out


def emulate(i, route, colsum=True):
    """dW / db in the kernel's summation order, on the CPU in fp32: 16-row MFMA steps, one accumulator per workgroup that walks its
    tiles in order (64-row tiles `tile = block + j * grid` for the streaming kernel, 128-row steps for the fallback), the
    workgroups' sums added one after the other.  dX and gm are the model's."""
    m = model(i, colsum)
    N, M, K = i["N"], i["M"], i["K"]
    grid, tile = (route[4], 64) if route[0] != "fallback" else (route[3], 128)
    rows = cdiv(N, tile * grid) * tile * grid
    a, b = torch.zeros(rows, M), torch.zeros(rows, K)
    a[:N], b[:N] = m["gm"], i["x"]
    spt = tile // 16
    steps = torch.bmm(a.view(-1, 16, M).transpose(1, 2), b.view(-1, 16, K)).view(-1, grid, spt, M, K)   # [round, block, step]
    ones = a.view(-1, grid, spt, 16, M).sum(3)                                                         # db: products with 1.0
    acc, accb = torch.zeros(grid, M, K), torch.zeros(grid, M)
    for rd in range(steps.shape[0]):
        for s in range(spt):
            acc, accb = acc + steps[rd, :, s], accb + ones[rd, :, s]
    dW = torch.zeros(M, K) if i["C0"] is None else i["C0"].clone()
    db = torch.zeros(M) if i["C0"] is None else i["cs0"].clone()
    for blk in range(grid):
        dW, db = dW + acc[blk], db + accb[blk]
    out = dict(m, dW=dW)
    if colsum:
        out["db"] = db
    return out


def ratios(got, mod, ref):
    return {k: row_ratio(got[k], mod[k], ref[k]) for k in TENSORS if k in ref and k in got}


# ---------------------------------------------------------------------------------------------
# mutations: kernel bugs in miniature.  name -> (applies(case), the tensors it may show in)
# ---------------------------------------------------------------------------------------------
MUTATIONS = {
    "drop_last_row": (lambda c: True, ("dW", "db")),                           # the last valid row is missing from the sums
    "row_past_n": (lambda c: True, ("dW", "db")),                              # row N is summed too (a range check one row long)
    "gutter_column": (lambda c: c["lda"] > c["M"], ("dW", "db")),              # the last column of a strided A read one to the right
    "mask_ge": (lambda c: c["act"] == 1, ("dW", "db", "dX", "gm")),            # relu mask y >= 0 instead of y > 0
    "xout_skipped_second_block": (lambda c: c["kind"] == "dense" and c["xout"] != 0 and c["N"] > 32, ("dX",)),   # rows 32-63 of a tile
    "bias_into_dw": (lambda c: c["colsum"], ("dW",)),                          # the ones column lands in dW[:, K - 1]
    "drop_tile": (lambda c: True, ("dW", "db")),                               # one 64-row tile is never summed
    # "g' rounded twice": the activation staging applied to a tile that already went through it — g'' = bf16(bf16(g s) s).  For the
    # relu mask that is the identity (the host test says so); for the shifted softplus every element shrinks by s in (1/2, 1).
    "staged_twice": (lambda c: c["act"] == 2, ("dW", "db", "dX", "gm")),
}


# ---------------------------------------------------------------------------------------------
# cases.  Every N is a few hundred rows at most except where a branch needs more; each names why it is the smallest shape that
# reaches its branch.  Keywords: cs (column sums / db), lda / ldb / ldy / lddx (row strides, default = width), aoff / boff /
# yoff (element offset of the base inside its NaN-filled buffer: 2 = 4-byte but not 16-byte aligned, 1 = 2-byte aligned),
# scratch (None, 0 or the byte offset past 16-byte alignment), det, prefill, ints, xout, gm.
# ---------------------------------------------------------------------------------------------
def _tn(N, M, K, act=0, cs=True, **kw):
    return dict(kind="tn", N=N, M=M, K=K, act=act, colsum=cs, xout=0, gm=False, **kw)


TN_CASES = {
    # the 16 streaming tile shapes; act rotates so that each of 0 / 1 / 2 runs in a 4-wave and in an 8-wave form; N from
    # {1, 33, 63, 64, 65, 96, 200}: one row, a second 32-row half of one row, one short of a tile, a tile, a tile and one row, a
    # tile and a half, three tiles and an 8-row rest
    "t11_k30": _tn(1, 30, 30, 0),                   # K = 30 + ones column: one tile
    "t12_k32": _tn(33, 32, 32, 1),                  # K = 32: the ones column opens a tile that holds nothing else
    "t14_k94": _tn(63, 30, 94, 2),                  # 95 columns: three tiles -> the 4-tile instantiation
    "t15_k128": _tn(64, 32, 128, 0),                # 129 columns: 5 tiles, 8 waves
    "t21": _tn(65, 34, 30, 1),
    "t22": _tn(96, 64, 34, 2),
    "t24_k96": _tn(200, 34, 96, 0),                 # 97 columns: four tiles proper
    "t25_k158": _tn(200, 64, 158, 1),               # the widest B with column sums
    "t41_m66": _tn(33, 66, 30, 2),                  # M = 66: three row tiles -> 4
    "t42": _tn(65, 96, 64, 0, cs=False),            # M = 96: the last shape of the 3 -> 4 bump
    "t44": _tn(96, 96, 96, 1, cs=False),            # both bumps, no ones column
    "t45_k160": _tn(63, 66, 160, 2, cs=False),      # K = 160: five full tiles, no room for the ones column
    "t51": _tn(64, 130, 30, 0),
    "t52": _tn(1, 160, 32, 1),
    "t54": _tn(200, 130, 94, 2),
    "t55": _tn(65, 160, 158, 0),
    "det200": _tn(200, 34, 34, 1, det=True),        # one workgroup takes four tiles, the last one partial; run twice: bit-equal
    "prefetch": _tn(16453, 34, 34, 0, ints=True),   # 257 tiles on 256 workgroups: block 0 prefetches a one-row tile
    "cap512": _tn((1 << 20) + 1, 2, 2, 0, ints=True),   # N >= 2^20: 512 workgroups, 33 tiles on block 0; integer inputs: exact
    "part_off": _tn(1984, 34, 34, 0, scratch=0),    # 31 tiles: scratch offered, atomics taken
    "part_on": _tn(1985, 34, 34, 0, scratch=0),     # 32 tiles: the scratch form + tn_reduce_kernel
    "part_on_bumped": _tn(2049, 66, 94, 1, scratch=0),   # ... with padding tiles on both sides of the reduce
    "scratch_misaligned": _tn(1985, 34, 34, 0, scratch=4),   # falls back to atomics
    "prefill": _tn(200, 34, 34, 0, prefill=True),   # C and colsum accumulate
    # strided operands at bases that are 4-byte but not 16-byte aligned; every gutter element and 70 rows past N are NaN
    "strided": _tn(65, 30, 30, 1, lda=36, ldb=40, ldy=32, aoff=2, boff=2, yoff=2),
    "strided_wide": _tn(200, 130, 126, 2, lda=136, ldb=136, ldy=132, aoff=2, boff=6, yoff=2),   # both staging loops (QA = 1, RA = 16)
    # the scalar-load fallback: its 8 instantiations, each reason for taking it
    "fb11_base2": _tn(200, 30, 30, 0, cs=False, lda=32, aoff=1),          # a 2-byte aligned base
    "fb21_odd_m": _tn(200, 33, 34, 0, cs=False),
    "fb31_odd_k": _tn(129, 96, 33, 0, cs=False),
    "fb41_odd_lda": _tn(200, 128, 64, 0, cs=False, lda=129),
    "fb12_k200": _tn(200, 30, 200, 0, cs=False),                          # more than 5 column tiles
    "fb22_k200": _tn(65, 34, 200, 0, cs=False),
    "fb32_k256": _tn(200, 66, 256, 0, cs=False),
    "fb42_k256": _tn(257, 128, 256, 0, cs=False),
    "fb51_m130_odd_lda": _tn(200, 130, 34, 0, cs=False, lda=131),         # five row tiles: two launches, <4,1> and <1,1> on columns 128, 129
}


def _dn(N, M, K, act, xout, db=True, gm=False, **kw):
    return dict(kind="dense", N=N, M=M, K=K, act=act, xout=xout, colsum=db, gm=gm, **kw)


DENSE_CASES = {
    # the nine tile shapes; act 1 / 2 in the 4-wave (no 5-tile side) and the 8-wave form, act 0 always 8 waves
    # N from {1, 32, 33, 64, 65, 97, 200}: at 32 the second dX block has remr = 0, at 33 and 97 a single row
    "d22": _dn(1, 34, 34, 0, 0),
    "d24_k66": _dn(32, 34, 66, 1, 1, gm=True),      # 67 columns: 3 -> 4
    "d25_k158": _dn(33, 34, 158, 2, 2),
    "d42_m66": _dn(64, 66, 34, 2, 0, db=False, gm=True),
    "d44_k94": _dn(65, 96, 94, 1, 2),
    "d44_nodb_k66": _dn(97, 66, 66, 0, 1, db=False),   # three column tiles without a bias column
    "d45_k160": _dn(97, 96, 160, 1, 0, db=False),
    "d52_m160": _dn(200, 160, 34, 2, 1),
    "d54": _dn(65, 160, 94, 0, 0, gm=True),
    "d55": _dn(200, 160, 158, 1, 2, gm=True),
    "d_strided": _dn(97, 66, 66, 2, 2, gm=True, lda=70, ldb=74, ldy=68, lddx=72, aoff=2, boff=2, yoff=6),
    "d_strided_relu": _dn(33, 34, 34, 1, 1, lda=40, ldb=36, ldy=38, lddx=40, aoff=6, boff=2, yoff=2),
    "d_det200": _dn(200, 34, 34, 1, 0, det=True),
    "d_part_off": _dn(1984, 34, 34, 0, 0, scratch=0),
    "d_part_on": _dn(1985, 34, 34, 2, 1, scratch=0, gm=True),
    "d_prefetch": _dn(16453, 34, 34, 1, 1, ints=True),
    "d_prefill": _dn(200, 34, 34, 0, 0, prefill=True),
}
for _c in list(TN_CASES.values()) + list(DENSE_CASES.values()):
    for _k, _v in dict(lda=_c["M"], ldb=_c["K"], ldy=_c["M"], lddx=_c["K"], aoff=0, boff=0, yoff=0, scratch=None, det=False,
                       prefill=False, ints=False).items():
        _c.setdefault(_k, _v)
CASES = {**TN_CASES, **DENSE_CASES}
# cases whose inputs are drawn from another seed so that every mutation meets the sensitivity condition
SEED_SHIFT = {}


def case_route(c, a_mod4=None, b_mod4=None, scratch_mod16="case"):
    """the route of a case; the GPU test passes the alignments of the pointers it actually hands over"""
    a_mod4 = (2 * c["aoff"]) % 4 if a_mod4 is None else a_mod4
    b_mod4 = (2 * c["boff"]) % 4 if b_mod4 is None else b_mod4
    scr = (None if c["scratch"] is None else c["scratch"] % 16) if scratch_mod16 == "case" else scratch_mod16
    if c["kind"] == "dense":
        return dense_route(c["M"], c["K"], c["colsum"], c["act"], c["N"], scr, c["det"])
    return tn_route(c["M"], c["K"], c["colsum"], c["act"], c["lda"], c["ldb"], a_mod4, b_mod4, c["N"], scr, c["det"])


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(spec, inputs, ref, model, route) of a named case; shared, read-only"""
    c = CASES[name]
    seed = 500 + sorted(CASES).index(name) + 1000 * SEED_SHIFT.get(name, 0)
    i = make_inputs(c["N"], c["M"], c["K"], c["act"], c["xout"], seed, ints=c["ints"], prefill=c["prefill"], dx=c["kind"] == "dense")
    return dict(spec=c, inputs=i, ref=reference64(i, c["colsum"]), model=model(i, c["colsum"]), route=case_route(c))


def mutated(name, mutation):
    c = case(name)
    return model(c["inputs"], c["spec"]["colsum"], mutation=mutation)


# ---------------------------------------------------------------------------------------------
# layer level: ops.linear / ops.linear_act on fp32 master weights, N = 130 rows (two tiles and two rows)
# ---------------------------------------------------------------------------------------------
LAYER_N = 130
# name -> (M, K, act, input gradient wanted, the launches expected).  A launch is ("dense", ldg, M, ldx, K, act, db) for
# mdl_dense_bwd_ex or ("tn", lda, M, ldb, K, act, colsum, byte offset of B's base past 16-byte alignment) for ops._gemm_tn
# (the launches of ops._tn_plan, made by ops._tn_dw_db; the route is chosen in ops._linear_backward).
LAYER_CASES = {
    "dense_relu": (66, 50, "relu", True, [("dense", 66, 66, 50, 50, 1, True)]),                  # ops._dense_bwd
    "dense_ssp": (130, 94, "ssp", True, [("dense", 130, 130, 94, 94, 2, True)]),
    "tn_act": (64, 114, "relu", False, [("tn", 64, 64, 114, 114, 1, True, 0)]),                  # no input gradient: mdl_gemm_tn_act
    "odd_m": (1, 64, None, True, [("tn", 2, 2, 64, 64, 0, True, 0)]),                            # M = 1 with bias: g padded to two columns
    "k258": (64, 258, None, True, [("tn", 64, 64, 258, 130, 0, True, 0), ("tn", 64, 64, 258, 128, 0, False, 4)]),   # kh = 130: db fused
    "k300": (64, 300, None, True, [("tn", 64, 64, 300, 150, 0, True, 0), ("tn", 64, 64, 300, 150, 0, False, 12)]),  # kh = 150: db fused
    "k320": (64, 320, None, True, [("tn", 64, 64, 320, 160, 0, False, 0), ("tn", 64, 64, 320, 160, 0, False, 0)]),  # kh = 160: library db
    "m162": (162, 64, None, True, [("tn", 64, 64, 162, 82, 0, False, 0), ("tn", 64, 64, 162, 80, 0, False, 4)]),    # transposed chunks
    "m450": (450, 100, None, True, [("tn", 100, 100, 450, 150, 0, False, 0), ("tn", 100, 100, 450, 150, 0, False, 12),
                                    ("tn", 100, 100, 450, 150, 0, False, 8)]),
}
LAYER_TENSORS = ("dW", "db", "dX")


def layer_inputs(M, K, seed):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    return dict(x=bfr(rnd(LAYER_N, K)), w=bfr(rnd(M, K) / K ** 0.5), b=bfr(rnd(M) * 0.1), gout=bfr(rnd(LAYER_N, M)))


def _act_fn(act):
    return {None: lambda v: v, "relu": torch.relu, "ssp": lambda v: torch.nn.functional.softplus(v) - LN2}[act]


def layer_reference64(x, w, b, gout, act, need_dx):
    """the whole layer under fp64 autograd: loss = sum(act(x W^T + b) * gout)"""
    p = {k: v.double().requires_grad_(True) for k, v in dict(x=x, w=w, b=b).items()}
    (_act_fn(act)(torch.nn.functional.linear(p["x"], p["w"], p["b"])) * gout.double()).sum().backward()
    out = dict(dW=p["w"].grad, db=p["b"].grad)
    if need_dx:
        out["dX"] = p["x"].grad
    return out


def layer_model(x, w, b, gout, act, need_dx):
    """The layer in fp32, rounded where the bf16 layer rounds: the saved output y = bf16(act(x W^T + b)) (fp32 accumulators, bias and
    activation on them, one rounding: csrc/linear.hip), then the backward of `model` from that y: g' from y, dW / db in fp32 from g',
    dX = bf16(g' W) — on every route (one-pass kernel, TN GEMM + streaming or library dX, column halves, transposed chunks)."""
    code = {None: 0, "relu": 1, "ssp": 2}[act]
    y = bfr(_act_fn(act)(x @ w.t() + b)) if code else None
    i = dict(N=x.shape[0], M=w.shape[0], K=w.shape[1], act=code, xout=0, g=gout, x=x, y=y, w=w if need_dx else None, C0=None, cs0=None)
    m = compute(i)
    return {k: m[k] for k in LAYER_TENSORS if k in m}


@functools.lru_cache(maxsize=None)
def layer_case(name):
    M, K, act, need_dx, calls = LAYER_CASES[name]
    i = layer_inputs(M, K, seed=700 + sorted(LAYER_CASES).index(name))
    return dict(inputs=i, act=act, need_dx=need_dx, calls=calls, ref=layer_reference64(act=act, need_dx=need_dx, **i),
                model=layer_model(act=act, need_dx=need_dx, **i), M=M, K=K)
