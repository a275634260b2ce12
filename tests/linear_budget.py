"""Error budget of the dense layers' FORWARD against an fp64 reference (helper module of test_linear_budget_host.py and
test_gpu_linear_budget.py; no test lives here).  It follows tests/dense_budget.py: the yardstick is a ROUNDING MODEL, the same
arithmetic in plain fp32 torch on the CPU, rounded to bf16 exactly where the kernel rounds.

One kernel body serves every case: linear_act_kernel (csrc/linear.hip), reached through
  mdl_linear_act         out = act(x W^T + b)                                                    entry "act"
  mdl_linear_act_in      the same on x := g .* act'(y), staged while the tile is loaded (XACT)   entry "in"
  mdl_linear_gather_act  + sum_t table_t[idx_t] before the activation (K6)                       entry "gather"
  mdl_linear_act_stats   + per-column (sum, sum of squares) of the rounded outputs about a shift entry "stats"
  mdl_linear_wide        out = x W^T for thousands of columns, 192 per workgroup                 entry "wide"
and from ops.linear_act / linear_gather_act / linear_relu_bn / matmul_wide                        LAYER_CASES

Measures:
  tight       row_ratio(got, model, ref64) <= ALLOWED["out"], rows = data rows.
  derived     s = the fp64 pre-activation, mag = sum|x||w| + |b| + sum|table|, terms = K + 1 + T, u = 2^-24:
              ANY fp32 evaluation order gives s^ with |s^ - s| <= delta = terms u / (1 - terms u) mag (bf16 x bf16 is exact
              in fp32), activation and rounding are monotone, so  bfr(act(s - delta)) <= got <= bfr(act(s + delta))  for every
              element.  Nothing in it is measured, and for most elements the interval is ONE bf16 value.  The shifted
              softplus goes through two hardware transcendentals: both ends move out by SSP_C u (1 + |s|).  XACT = 2 rounds
              the staged operand and takes the tight measure only.
  statistics  the 16 replicas of (sum, sum of squares) added in fp64 against fp64 sums over the kernel's OWN stored rows:
              |S0 - sum(y - sh)| <= (n + 18) u sum|y - sh|,  |S1 - sum(y - sh)^2| <= (n + 19) u sum(y - sh)^2  (stats_check).
  memory      operands lie in NaN, outputs are carved out of NaN (test_gpu_linear_budget.py).

The table of measured values per case stands in front of ALLOWED below.
"""
import functools

import torch

from cgconv_budget import bfr, fmt, row_ratio, row_rms  # noqa: F401  (re-exported for the tests)

LN2 = 0.6931471805599453
PAD_ROWS = 70                                    # NaN rows behind x, y, g and behind every output (more than one tile)
GUARD = 256                                      # bytes behind every output in the arenas of the GPU test
U = 2.0 ** -24                                   # unit roundoff of fp32
REPLICAS = 16                                    # MDL_BN_REPLICAS: copies of the (sum, sum of squares) row pair
SUMS_ROWS = 2 * REPLICAS + 2                     # mdl_bn_sums_rows(): replicas, then the two totals rows; the shift row follows
TABLE_ROWS = 9                                   # valid rows of every gathered table; row TABLE_ROWS is all NaN

# Permitted row_ratio: twice the largest value measured on the MI355X over every case of test_gpu_linear_budget.py and its runs
# (three), rounded up to one decimal, never below 2 and never above 5.  The output has no atomics and is the same bits in every
# launch; the factor 2 covers what kernel and model draw differently: the summation order, which decides the rare element whose
# fp32 value lies within its noise of a bf16 tie, and through those elements the last digits of mean and var.
# Measured on the MI355X (one run; `largest` is over three): per case the route, row_ratio against the rounding model, how many
# elements are bit-equal to the model, the share of elements whose derived interval is a single bf16 value (every element of every
# case lay inside its interval), for act = 2 the smallest SSP_C that would admit every element (`ssp`), and for the statistics
# forms f0 / f1 = the largest |S - exact| as a fraction of its derived bound, sh = bf16 steps between the shift and output row 0,
# and the row_ratio of mean and var.  Layer level: linear_relu_bn's z, running_mean, running_var as fractions of their tolerances.
#   case              route                                     measures
#   p64_1_k4_m1       lin <64,1,0,0,0> NW8 grid 1               ratio 1.0000  equal 1/1  single 1.0000
#   p64_2_k62_m33     lin <64,2,0,0,0> NW8 grid 1               ratio 1.0000  equal 1023/1023  single 0.9795
#   p64_4             lin <64,4,0,0,0> NW8 grid 1               ratio 1.0000  equal 2111/2112  single 0.9645  ssp 0.00 u
#   p64_5_k4          lin <64,5,0,0,0> NW8 grid 1               ratio 1.0000  equal 4290/4290  single 0.9984
#   p128_1_k66        lin <128,1,0,0,0> NW8 grid 1              ratio 1.0000  equal 2016/2016  single 0.9841
#   p128_2            lin <128,2,0,0,0> NW8 grid 1              ratio 1.0000  equal 4096/4096  single 0.9209  ssp 0.00 u
#   p128_4_k66        lin <128,4,0,0,0> NW8 grid 2              ratio 1.0000  equal 8320/8320  single 0.9632
#   p128_5            lin <128,5,0,0,0> NW8 grid 2              ratio 1.0000  equal 15520/15520  single 0.9616
#   p160_1_k130_m1    lin <160,1,0,0,0> NW4 grid 4              ratio 1.0000  equal 200/200  single 0.9250  ssp 0.00 u
#   p160_2            lin <160,2,0,0,0> NW4 grid 1              ratio 1.0000  equal 64/64  single 0.8750
#   p160_4_k130       lin <160,4,0,0,0> NW4 grid 1              ratio 1.0000  equal 2178/2178  single 0.9564
#   p160_5            lin <160,5,0,0,0> NW4 grid 2              ratio 1.0000  equal 8449/8450  single 0.9031  ssp 0.00 u
#   p256_1_k162       lin <256,1,0,0,0> NW8 grid 1              ratio 1.0000  equal 992/992  single 0.9113  ssp 0.00 u
#   p256_2_m33        lin <256,2,0,0,0> NW8 grid 2              ratio 1.0000  equal 3201/3201  single 0.9047
#   p256_4_k162       lin <256,4,0,0,0> NW8 grid 4              ratio 1.0000  equal 25597/25600  single 0.8979
#   in_x4             lin <64,2,0,0,0> NW8 grid 1               ratio 1.0000  equal 4032/4032  single 0.9774
#   ints200           lin <256,4,0,0,0> NW8 grid 4              ratio 0.0000  equal 25600/25600  single 0.9557
#   cap512            lin <64,2,0,0,0> NW8 grid 512             ratio 0.0000  equal 1114146/1114146  single 0.9376
#   g1_64_1           lin <64,1,1,0,0> NW4 grid 1               ratio 1.0000  equal 32/32  single 1.0000
#   g1_128_2          lin <128,2,1,0,0> NW4 grid 1              ratio 1.0000  equal 2112/2112  single 0.9631  ssp 0.00 u
#   g1_160_4          lin <160,4,1,0,0> NW4 grid 2              ratio 1.0000  equal 4290/4290  single 0.9093
#   g1_256_1_m1       lin <256,1,1,0,0> NW4 grid 2              ratio 1.0000  equal 97/97  single 0.8866  ssp 0.00 u
#   g2_64_2_k4        lin <64,2,2,0,0> NW4 grid 4               ratio 1.0000  equal 6600/6600  single 0.9965  ssp 0.00 u
#   g2_128_4          lin <128,4,2,0,0> NW4 grid 1              ratio 1.0000  equal 3968/3968  single 0.9592
#   g2_160_1          lin <160,1,2,0,0> NW4 grid 1              ratio 1.0000  equal 2048/2048  single 0.9673
#   g2_256_2_k162     lin <256,2,2,0,0> NW4 grid 1              ratio 1.0000  equal 2112/2112  single 0.9058
#   g3_64_4           lin <64,4,3,0,0> NW4 grid 1               ratio 1.0000  equal 8064/8064  single 0.9634
#   g3_128_1          lin <128,1,3,0,0> NW4 grid 1              ratio 1.0000  equal 32/32  single 0.9688
#   g3_160_2          lin <160,2,3,0,0> NW4 grid 1              ratio 1.0000  equal 1088/1088  single 0.9072  ssp 0.00 u
#   g3_256_4          lin <256,4,3,0,0> NW4 grid 4              ratio 1.0000  equal 13200/13200  single 0.9178
#   g_ints            lin <128,4,2,0,0> NW4 grid 2              ratio 0.0000  equal 6402/6402  single 0.9517
#   x1_64_5           lin <64,5,0,1,0> NW8 grid 2               ratio 1.0000  equal 10400/10400  single 0.9764
#   x1_128_1          lin <128,1,0,1,0> NW8 grid 1              ratio 1.0000  equal 1056/1056  single 0.9669
#   x1_160_2          lin <160,2,0,1,0> NW4 grid 4              ratio 1.0000  equal 12799/12800  single 0.9381  ssp 0.00 u
#   x1_256_4          lin <256,4,0,1,0> NW8 grid 2              ratio 1.0000  equal 12415/12416  single 0.8766
#   x2_64_2           lin <64,2,0,2,0> NW8 grid 1               ratio 1.0000  equal 1054/1054
#   x2_128_4          lin <128,4,0,2,0> NW8 grid 1              ratio 1.0000  equal 4224/4224
#   x2_160_5          lin <160,5,0,2,0> NW4 grid 1              ratio 1.0000  equal 130/130
#   x2_256_1          lin <256,1,0,2,0> NW8 grid 4              ratio 1.0000  equal 6400/6400
#   s64_2_k4_m34      lin <64,2,0,0,1> NW8 grid 4               ratio 1.0000  equal 6800/6800  single 0.9991  f0 0 f1 0.00371 sh 0  mean 0.9998 var 1.0000
#   s64_4             lin <64,4,0,0,1> NW8 grid 2               ratio 1.0000  equal 6402/6402  single 0.9686  f0 0.00236 f1 0.0141 sh 0  mean 0.9999 var 1.0000
#   s64_5_m160        lin <64,5,0,0,1> NW8 grid 2               ratio 1.0000  equal 15520/15520  single 0.9812  f0 0.00519 f1 0.0131 sh 0  mean 1.0000 var 0.9999
#   s128_2            lin <128,2,0,0,1> NW8 grid 4              ratio 1.0000  equal 12799/12800  single 0.9641  ssp 0.00 u  f0 0.00287 f1 0.0339 sh 0  mean 1.0000 var 0.9999
#   s128_4            lin <128,4,0,0,1> NW8 grid 1              ratio 1.0000  equal 8063/8064  single 0.9618  f0 0.0101 f1 0.0422 sh 0  mean 0.9999 var 1.0000
#   s128_5            lin <128,5,0,0,1> NW8 grid 1              ratio 1.0000  equal 4290/4290  single 0.9627  f0 0 f1 0 sh 0  mean 1.0000 var 0.0000
#   s160_2_many       lin <160,2,0,0,1> NW4 grid 18             ratio 1.0000  equal 37025/37026  single 0.9503  f0 5.32e-05 f1 0.000586 sh 0  mean 1.0002 var 1.0001
#   s160_4_far        lin <160,4,0,0,1> NW4 grid 4              ratio 1.0000  equal 13199/13200  single 0.9626  f0 0.00123 f1 0.0131 sh 0  mean 1.0032 var 1.0029
#   s160_5_k160_m160  lin <160,5,0,0,1> NW4 grid 1              ratio 1.0000  equal 10239/10240  single 0.8998  ssp 0.00 u  f0 0.0102 f1 0.0435 sh 0  mean 0.9999 var 0.9999
#   sg64_2            lin <64,2,2,0,1> NW4 grid 2               ratio 1.0000  equal 2210/2210  single 0.9873  f0 0 f1 0.0119 sh 0  mean 1.0000 var 0.9999
#   sg64_4_k4         lin <64,4,2,0,1> NW4 grid 4               ratio 1.0000  equal 25600/25600  single 0.9985  f0 0 f1 0.0222 sh 0  mean 1.0000 var 1.0000
#   sg128_2           lin <128,2,2,0,1> NW4 grid 1              ratio 1.0000  equal 64/64  single 0.9375  f0 0 f1 0 sh 0  mean 1.0000 var 0.0000
#   sg128_4           lin <128,4,2,0,1> NW4 grid 2              ratio 1.0000  equal 6402/6402  single 0.9647  ssp 0.00 u  f0 0.00234 f1 0.0211 sh 0  mean 0.9999 var 0.9999
#   sg160_2           lin <160,2,2,0,1> NW4 grid 1              ratio 1.0000  equal 2112/2112  single 0.9626  f0 0 f1 0 sh 0  mean 1.0000 var 0.0000
#   sg160_4_far       lin <160,4,2,0,1> NW4 grid 4              ratio 1.0000  equal 25600/25600  single 0.9521  f0 0 f1 0.0183 sh 0  mean 1.0003 var 0.9999
#   w64_1blk_192      wide kp64 blocks 1 last 192 chunks 7      ratio 1.0000  equal 86015/86016  single 0.9672
#   w128_2blk_1       wide kp128 blocks 2 last 1 chunks 8 xcd   ratio 1.0000  equal 86655/86657  single 0.9193
#   w160_4blk_191     wide kp160 blocks 4 last 191 chunks 2     ratio 1.0000  equal 49853/49855  single 0.8964
#   w64_rounds        wide kp64 blocks 2 last 1 chunks 64 xcd   ratio 1.0000  equal 790721/790721  single 0.9967
#   w160_xcd_4blk     wide kp160 blocks 4 last 192 chunks 16 xcd ratio 1.0000  equal 786408/786432  single 0.9179
#   w_ints            wide kp64 blocks 3 last 1 chunks 9        ratio 0.0000  equal 197505/197505  single 0.9347
#   act_relu          1 launch(es): mdl_linear_act              ratio 1.0000  equal 6500/6500  single 0.9843
#   act_ssp           1 launch(es): mdl_linear_act              ratio 1.0000  equal 8579/8580  single 0.9240
#   act_none          1 launch(es): mdl_linear_act              ratio 1.0000  equal 4290/4290  single 0.9646
#   gather_1          1 launch(es): mdl_linear_gather_act       ratio 1.0000  equal 8320/8320  single 0.9851
#   gather_2          1 launch(es): mdl_linear_gather_act       ratio 1.0000  equal 13000/13000  single 0.9625
#   gather_3          1 launch(es): mdl_linear_gather_act       ratio 1.0000  equal 4160/4160  single 0.9524
#   bn_0              1 launch(es): mdl_linear_act_stats        z 0.739  running_mean 0.00059  running_var 0.0035
#   bn_2              1 launch(es): mdl_linear_act_stats        z 0.692  running_mean 0.00054  running_var 0.00098
#   bn_1              2 launch(es): mdl_linear_gather_act       z 0.727  running_mean 0.00056  running_var 0.0025
#   bn_3              2 launch(es): mdl_linear_gather_act       z 0.704  running_mean 0.00085  running_var 0.002
#   bn_0_det          2 launch(es): mdl_linear_act              z 0.754  running_mean 0.00056  running_var 0.0028
#   bn_2_det          2 launch(es): mdl_linear_gather_act       z 0.793  running_mean 0.0009  running_var 0.0018
#   wide              1 launch(es): mdl_linear_wide             ratio 1.0000  equal 656380/656384  single 0.9843
#   dx_relu           dX: mdl_linear_act_in                     ratio 1.0000  equal 8320/8320
#   dx_ssp            dX: mdl_linear_act_in                     ratio 1.0000  equal 8320/8320
# largest: out 1.0000, mean 1.0032 (s160_4_far), var 1.0029 (s160_4_far); of the statistics bounds f0 0.010, f1 0.044
# (s160_5_k160_m160); ssp 0.00 everywhere: no element needed the transcendentals' term.  4,211,710 of 4,211,756 elements were
# bit-equal to the model; the 46 others lie in intervals that hold two values.  The smallest single-valued share was 0.875
# (p160_2: 64 elements).  0.0000: integer inputs, model and kernel both exact.  1.0000: the one rounding of the output dominates
# both sides.  No case failed: the forward's dispatch, staging maps, tile clamps, table packing and both tile maps of the wide
# form hold at every edge this suite reaches.
ALLOWED = {"out": 2.0, "mean": 2.1, "var": 2.1}
# The absolute term of the derived interval for act = 2, in units of u (1 + |s|): four times the largest deviation of the fp32
# CPU model's own shifted softplus from fp64 over every ssp case (1.494 units, case sg128_4: test_linear_budget_host.py measures
# it again), rounded up to one decimal.  It only matters where |out| < about 2^-12: everywhere else half a bf16 step of the
# output is thousands of these units.
SSP_C = 6.0


def cdiv(a, b):
    return -(-a // b)


# ---------------------------------------------------------------------------------------------
# the dispatch, restated: the kernel choice is made in C and is not observable from Python
# ---------------------------------------------------------------------------------------------
def lin_route(entry, N, K, M, tables=0, xact=0, stats=False, *, orphan=False, act=0, x_mod16=0, w_mod4=0, out_mod2=0, y_mod4=0):
    """The kernel an entry point of csrc/linear.hip launches, from what the caller passes (tables = how many of p1 / p2 / p3 are
    not null, orphan = a table comes without its index, *_mod* = a base address modulo its required alignment).
      ("lin", kp, nt, G, X, S, NW, grid)  linear_act_kernel<kp, nt, G, X, S> with 64 NW threads on `grid` workgroups:
                                          kp, nt lines 405-406; NW = MDL_LIN_NW (line 26); grid lines 407-408 (LIN_GRID, line 30)
      ("unsupp" | "arg", why)             MDL_E_UNSUPP / MDL_E_ARG with a fragment of the error text
      ("empty",)                          N = 0: MDL_OK, nothing launched
    The checks are in the order of the MDL_REQUIRE lines of the entry point:
      act / gather  mdl_linear_gather_act, lines 359-375 (mdl_linear_act forwards to it without tables, line 333)
      in            mdl_linear_act_in, lines 343-352
      stats         mdl_linear_act_stats, lines 382-397, then the statistics branch of linear_launch, lines 425-430"""
    assert entry in ("act", "in", "gather", "stats") and stats == (entry == "stats")
    assert (tables == 0 or entry in ("gather", "stats")) and (xact == 0 or entry == "in")
    shape = 4 <= K <= 256 and K % 2 == 0 and 1 <= M <= 160 and (M <= 128 or K <= 160)
    if entry == "in":
        if not 0 <= xact <= 2 or (xact and y_mod4):
            return ("arg", "xact must be 0, 1 (relu) or 2")                                   # line 344
        if not shape:
            return ("unsupp", "need even 4<=K<=256 and 1<=M<=160")                            # line 346
        if not 0 <= act <= 2:
            return ("arg", "act must be 0")                                                   # line 348
        if N < 0:
            return ("arg", "bad arguments")                                                   # line 349
        if x_mod16 % 4 or w_mod4:
            return ("arg", "misaligned pointer")                                              # line 350
    elif entry in ("act", "gather"):
        if orphan:
            return ("arg", "table without index")                                             # line 360
        if tables and M > 128:
            return ("unsupp", "gathered tables need M <= 128")                                # line 361
        if not shape:
            return ("unsupp", "need even 4<=K<=256 and 1<=M<=160")                            # line 368
        if not 0 <= act <= 2:
            return ("arg", "act must be 0")                                                   # line 370
        if N < 0:
            return ("arg", "bad arguments")                                                   # line 371
        if x_mod16 or w_mod4 or out_mod2:
            return ("arg", "misaligned pointer")                                              # line 372
    else:
        if orphan:
            return ("arg", "table without index")                                             # line 384
        if not (4 <= K <= 160 and K % 2 == 0 and 34 <= M <= 160 and M % 2 == 0 and (not tables or M <= 128)):
            return ("unsupp", "need even 4<=K<=160 and even 34<=M<=160")                      # line 390
        if not 0 <= act <= 2:
            return ("arg", "act must be 0")                                                   # line 392
        if N < 0:
            return ("arg", "bad arguments")                                                   # line 393
        if x_mod16 or w_mod4 or out_mod2:
            return ("arg", "misaligned pointer")                                              # line 394
    if N == 0:
        return ("empty",)                                                                     # lines 351, 374, 396
    kp = 64 if K <= 64 else (128 if K <= 128 else (160 if K <= 160 else 256))                 # line 405
    nt = 1 if M <= 32 else (2 if M <= 64 else (4 if M <= 128 else 5))                         # line 406
    if stats and (kp > 160 or nt < 2 or tables not in (0, 2) or (tables and nt > 4)):
        return ("unsupp", "unsupported shape")                                                # line 427
    nw = 4 if kp == 160 or tables else 8                                                      # line 26
    return ("lin", kp, nt, tables, xact, stats, nw, min(cdiv(N, 64), 512))


def wide_route(N, K, M, *, x_mod16=0, w_mod4=0, out_mod2=0):
    """mdl_linear_wide (csrc/linear.hip:487-513): ("wide", kp, blocks, last_width, chunks, xcd_map) — linear_act_kernel<kp, 6, 0, 0>
    on a (blocks, chunks) grid: blocks of 32 WIDE_NT = 192 columns (line 497), at most 64 row chunks (lines 498-499), the
    XCD-aware tile map where the chunks are a multiple of 8 (line 68)."""
    if not (4 <= K <= 160 and K % 2 == 0 and 1 <= M <= 192 * 65535 and M * 2 * 64 < 0x7fffffff):
        return ("unsupp", "need even 4<=K<=160")                                              # line 490
    if N < 0:
        return ("arg", "bad arguments")                                                       # line 492
    if x_mod16 or w_mod4 or out_mod2:
        return ("arg", "misaligned pointer")                                                  # line 493
    if N == 0:
        return ("empty",)                                                                     # line 495
    kp = 64 if K <= 64 else (128 if K <= 128 else 160)                                        # line 496
    blocks, chunks = cdiv(M, 192), min(cdiv(N, 64), 64)
    return ("wide", kp, blocks, M - 192 * (blocks - 1), chunks, chunks % 8 == 0)


def route_label(route):
    if route[0] == "wide":
        return "wide kp%d blocks %d last %d chunks %d%s" % (route[1], route[2], route[3], route[4], " xcd" if route[5] else "")
    return "lin <%d,%d,%d,%d,%d> NW%d grid %d" % (route[1], route[2], route[3], route[4], int(route[5]), route[6], route[7])


# ---------------------------------------------------------------------------------------------
# bf16 neighbours
# ---------------------------------------------------------------------------------------------
def _ordered(t):
    b = t.to(torch.bfloat16).view(torch.int16).to(torch.int32)
    return torch.where(b >= 0, b, -(b & 0x7fff))


def bf_step(t, k):
    """the bf16 value k steps above (k < 0: below) the bf16-valued fp32 tensor t"""
    o = _ordered(t) + k
    b = torch.where(o >= 0, o, (-o) | 0x8000)
    return ((b & 0xffff) - ((b & 0x8000) << 1)).to(torch.int16).view(torch.bfloat16).to(torch.float32)


# ---------------------------------------------------------------------------------------------
# inputs, fp64 reference, rounding model
# ---------------------------------------------------------------------------------------------
def act_fn(code, v):
    if code == 1:
        return torch.relu(v)
    if code == 2:
        return torch.nn.functional.softplus(v) - LN2
    return v


def dact(code, v, dtype):
    """act'(.) as a function of the activation's OUTPUT: relu v > 0, shifted softplus 1 - exp(-(v + ln 2))"""
    v = v.to(dtype)
    if code == 1:
        return (v > 0).to(dtype)
    if code == 2:
        return 1.0 - torch.exp(-(v + LN2))
    return torch.ones_like(v)


def make_inputs(c, seed):
    """fp32 tensors that are exact in bf16.  x [N, K] ~ N(0, 1) (XACT: g ~ N(0, 1) and y = relu(2 N(0, 1)) with exact zeros for
    XACT = 1, ssp(2 N(0, 1)) for XACT = 2), w [M, K] ~ N(0, 1 / K), b [M] ~ 0.5 N(0, 1), tables [TABLE_ROWS, M] ~ 0.5 N(0, 1),
    idx [N] int32 (`idx`: "rand", "equal": every entry the same row, "last": every second entry the last valid row).  One more
    row of x / g / y (`*_pad`) stands for what lies behind the arrays: only a mutation reads it.
    ints: x, w, b, tables integers in {-3 .. 3}: every partial sum is an integer below 2^24, so the fp32 result is EXACT in any
    order and the kernel must be bit-equal to the model.
    far: column 1 has bias 40 and weights 0.1 / sqrt(K): a BatchNorm column whose mean is far above its spread."""
    N, K, M = c["N"], c["K"], c["M"]
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    if c["ints"]:
        assert c["act"] in (0, 1) and c["xact"] == 0, "a softplus factor is no integer"
        q = lambda t: t.round().clamp(-3, 3)
    else:
        q = bfr
    i = dict(spec=c, x=None, g=None, y=None)
    rows = q(rnd(N + 1, K))
    if c["xact"]:
        y = bfr(act_fn(c["xact"], rnd(N + 1, K) * 2.0))
        i.update(g=rows[:N], g_pad=rows[N:], y=y[:N], y_pad=y[N:])
    else:
        i.update(x=rows[:N], x_pad=rows[N:])
    i["w"] = q(rnd(M, K) * (1.0 if c["ints"] else K ** -0.5))
    i["b"] = q(rnd(M) * (1.0 if c["ints"] else 0.5)) if c["bias"] else None
    if c["far"]:
        i["w"][1], i["b"][1] = bfr(i["w"][1] * 0.1), 40.0
    i["tables"] = [q(rnd(TABLE_ROWS, M) * (1.0 if c["ints"] else 0.5)) for _ in c["slots"]]
    if c["far"]:
        for tab in i["tables"]:
            tab[:, 1] = bfr(tab[:, 1] * 0.1)
    idx = []
    for t in range(len(c["slots"])):
        ix = torch.randint(0, TABLE_ROWS, (N,), generator=gen, dtype=torch.int32)
        if c["idx"] == "equal":
            ix[:] = int(ix[0])
        if c["idx"] == "last":
            ix[t % 2::2] = TABLE_ROWS - 1
        idx.append(ix)
    i["idx"] = idx
    return i


def n_true_of(c):
    """max(1, min(*n_dev, N)) (csrc/linear.hip:170); a null n_dev counts every row"""
    return c["N"] if c["nd"] is None else max(1, min(c["nd"], c["N"]))


def _kp(K, wide=False):
    return 64 if K <= 64 else (128 if K <= 128 else (160 if K <= 160 or wide else 256))


def compute(i, dtype=torch.float32, rounded=True, mutation=None):
    """dict(out [N, M], pre = the unrounded value behind out[, sh, S0, S1, mean, var [M]]) of one case in `dtype`; rounded: round
    to bf16 where the kernel does; mutation: a key of MUTATIONS"""
    c = i["spec"]
    N, K, M, act, wide = c["N"], c["K"], c["M"], c["act"], c["entry"] == "wide"
    r = bfr if rounded else (lambda t: t)

    def staged(x, g, y):
        if not c["xact"]:
            return x.to(dtype)
        if c["xact"] == 1:
            return g.to(dtype) * ((y >= 0) if mutation == "mask_ge" else (y > 0)).to(dtype)
        v = r(g.to(dtype) * dact(2, y, dtype))
        return r(v * dact(2, y, dtype)) if mutation == "staged_twice" else v
    x = staged(i["x"], i["g"], i["y"])
    if mutation == "row_past_n":
        x = torch.cat([x, staged(i.get("x_pad"), i.get("g_pad"), i.get("y_pad"))])
    rows = x.shape[0]
    kp = _kp(K, wide)
    if mutation == "k_tail_dropped":
        x = x.clone()
        x[:, 128 * (kp // 128):] = 0
    if mutation == "last_kstep_dropped":
        x = x.clone()
        x[:, kp - 16:] = 0
    w = i["w"].to(dtype)
    if mutation == "wide_block_shifted":
        w = w[(torch.arange(M) + 192) % M]
    pre = x @ w.t()
    if i["b"] is not None:
        b = i["b"].to(dtype)
        pre = pre + (b[torch.arange(M) % 32] if mutation == "bias_of_block0" else b)
    bare = pre
    if mutation == "act_before_tables":
        pre = act_fn(act, pre)
    tabs = list(zip(i["tables"], i["idx"]))
    if mutation == "table_dropped":
        tabs = tabs[:-1]
    for tab, ix in tabs:
        ix = torch.cat([ix, ix[-1:]])[:rows].long()          # (row N of a mutation gathers like row N - 1: the kernel's clamp)
        if mutation == "table_rows_permuted":
            n = torch.arange(rows)
            swap = n ^ 4
            ix = ix[torch.where(swap < rows, swap, n)]
        pre = pre + tab.to(dtype)[ix]
    val = pre if mutation == "act_before_tables" else act_fn(act, pre)
    res = dict(out=r(val), pre=val)
    if c["entry"] == "stats":
        y, n = res["out"][:N], n_true_of(c)
        sh = y[0]
        rows_in = torch.arange(N) < (N if mutation == "stats_counts_padding" else n)
        if mutation == "stats_half_dropped":
            rows_in = rows_in & ((torch.arange(N) % 8) < 4)
        d = ((val[:N] if mutation == "stats_unrounded" else y) - sh) * rows_in.to(dtype)[:, None]
        S0, S1 = d.sum(0), (d * d).sum(0)
        res.update(S0=S0, S1=S1, mean=sh + S0 / n, var=S1 / n - (S0 / n) ** 2)
        res["sh"] = r(act_fn(act, bare[0])) if mutation == "shift_without_tables" else sh
    return res


def reference64(i):
    """out = act(x W^T + b + sum_t table_t[idx_t]) in fp64 with nothing rounded (XACT: x := g .* act'(y)); the statistics are those
    of these fp64 rows n < n_true"""
    return compute(i, torch.float64, rounded=False)


def model(i, mutation=None):
    """The kernel in plain fp32 torch, rounded where it rounds (csrc/linear.hip):
      x'    XACT = 1: the mask y > 0 on the bf16 g, exact (line 156); XACT = 2: g (1 - exp(-(y + ln 2))) in fp32, rounded to bf16
            once as it is staged (lines 158-160)
      out   fp32 sums of exact products on accumulators that start at the bias (line 236), the gathered table rows added in fp32
            (line 270), the activation on the fp32 value (lines 290-294), ONE rounding to bf16 (line 295)
      stats sums of (rounded output - shift) and its square over the rows n < n_true (lines 297-299), the shift = the bf16-rounded
            output row 0 (lines 177-194)"""
    return compute(i, torch.float32, rounded=True, mutation=mutation)


def preact64(i):
    """(s, delta) of the derived measure: the fp64 pre-activation of the operands the kernel multiplies (XACT = 1: the masked g,
    exact) and delta = terms u / (1 - terms u) (sum|x||w| + |b| + sum|table|), terms = K + 1 + T, widened by a relative 2^-30"""
    c = i["spec"]
    assert c["xact"] != 2
    x = (i["x"] if not c["xact"] else i["g"] * (i["y"] > 0)).double()
    w = i["w"].double()
    s, mag = x @ w.t(), x.abs() @ w.abs().t()
    if i["b"] is not None:
        s, mag = s + i["b"].double(), mag + i["b"].double().abs()
    for tab, ix in zip(i["tables"], i["idx"]):
        s, mag = s + tab.double()[ix.long()], mag + tab.double()[ix.long()].abs()
    terms = c["K"] + 1 + len(i["tables"])
    return s, terms * U / (1 - terms * U) * mag * (1 + 2.0 ** -30)


def interval(i, c_ssp=None):
    """(lo, hi): the bf16 values between which every output element must lie"""
    act = i["spec"]["act"]
    s, delta = preact64(i)
    a = (SSP_C if c_ssp is None else c_ssp) * U * (1 + s.abs()) if act == 2 else 0.0
    return bfr(act_fn(act, s - delta) - a), bfr(act_fn(act, s + delta) + a)


def interval_report(got, i):
    """dict(inside = share of elements inside the interval, single = share whose interval is one bf16 value, ssp_units = for
    act = 2 the smallest SSP_C that would admit every element (0: the transcendentals' term was not needed))"""
    lo, hi = interval(i)
    rep = dict(inside=float(((got >= lo) & (got <= hi)).double().mean()), single=float((lo == hi).double().mean()), ssp_units=0.0)
    if i["spec"]["act"] == 2:
        s, delta = preact64(i)
        # the reals that round to `got` lie between the midpoints to its bf16 neighbours
        cell_lo, cell_hi = (got.double() + bf_step(got, -1).double()) / 2, (got.double() + bf_step(got, 1).double()) / 2
        need = torch.maximum(cell_lo - act_fn(2, s + delta), act_fn(2, s - delta) - cell_hi).clamp(min=0)
        rep["ssp_units"] = float((need / (U * (1 + s.abs()))).max())
    return rep


def ssp_model_units(i):
    """the largest deviation of the CPU's fp32 shifted softplus from fp64, in units of u (1 + |s|), on the fp32 value of s"""
    s, _ = preact64(i)
    return float(((act_fn(2, s.float()).double() - act_fn(2, s)).abs() / (U * (1 + s.abs()))).max())


def stats_check(out, sh, S0, S1, n):
    """The derived statistics bounds against fp64 sums over the kernel's own stored rows `out[:n]`:
    dict(f0, f1 = the largest |S - exact| as a fraction of its bound (inf: a sum of zeros is not zero), sh_steps = how many bf16
    steps the shift lies from the stored output row 0, at most)"""
    d = out[:n].double() - sh.double()
    e0, m0, e1 = d.sum(0), d.abs().sum(0), (d * d).sum(0)

    def frac(S, exact, bound):
        err = (S.double() - exact).abs()
        f = torch.where(bound > 0, err / bound.clamp(min=1e-300), torch.where(err == 0, torch.zeros_like(err), torch.full_like(err, float("inf"))))
        return float(f.max())
    steps = 0 if torch.equal(sh, out[0]) else (1 if bool(((sh == out[0]) | (sh == bf_step(out[0], 1)) | (sh == bf_step(out[0], -1))).all()) else 2)
    return dict(f0=frac(S0, e0, (n + 18) * U * m0), f1=frac(S1, e1, (n + 19) * U * e1), sh_steps=steps)


# ---------------------------------------------------------------------------------------------
# mutations: kernel bugs in miniature.  name -> (applies(case), measure that owns it, the tensors it may show in)
# measures: "out" the tight ratio and the interval, "memory" a row past N is written, "stats" the statistics bounds / the shift
# ---------------------------------------------------------------------------------------------
def _is(c, *entries):
    return c["entry"] in entries


MUTATIONS = {
    # the dwords past 64 Q of a row are not staged (Q = KP / 128: KP = 64 stages nothing, KP = 160 loses columns 128 ..)
    "k_tail_dropped": (lambda c: _kp(c["K"], _is(c, "wide")) in (64, 160) and c["K"] > 128 * (_kp(c["K"], _is(c, "wide")) // 128), "out"),
    "last_kstep_dropped": (lambda c: c["K"] > _kp(c["K"], _is(c, "wide")) - 16, "out"),          # the last 16 columns are left out of the sum
    "row_past_n": (lambda c: True, "memory"),                                                   # row N is staged and stored
    "bias_of_block0": (lambda c: c["bias"] and c["M"] > 32, "out"),                              # bias[col % 32]
    "table_dropped": (lambda c: len(c["slots"]) > 0, "out"),                                     # the last table is not added
    "table_rows_permuted": (lambda c: len(c["slots"]) > 0 and c["N"] > 4 and c["idx"] != "equal", "out"),   # rows r and r ^ 4 swap
    "act_before_tables": (lambda c: len(c["slots"]) > 0 and c["act"] != 0, "out"),
    "mask_ge": (lambda c: c["xact"] == 1, "out"),                                                # relu mask y >= 0
    "staged_twice": (lambda c: c["xact"] == 2, "out"),                                           # the XACT = 2 staging applied twice
    "wide_block_shifted": (lambda c: _is(c, "wide") and c["M"] > 192, "out"),                    # a column block takes the next one's weights
    # (the bound grows with n^2 and the rounding noise with sqrt(n): the unrounded sums stand over it up to a few hundred rows)
    "stats_unrounded": (lambda c: _is(c, "stats") and 30 <= n_true_of(c) <= 300, "stats"),
    "stats_counts_padding": (lambda c: _is(c, "stats") and n_true_of(c) < c["N"], "stats"),      # rows >= n_true are counted
    "stats_half_dropped": (lambda c: _is(c, "stats") and n_true_of(c) > 4, "stats"),             # the h = 1 rows (row % 8 >= 4) are missing
    "shift_without_tables": (lambda c: _is(c, "stats") and len(c["slots"]) > 0, "stats"),        # the stored shift is not the one used
}


# ---------------------------------------------------------------------------------------------
# cases.  Each names why it is the smallest shape that reaches its branch.  Keywords: bias, slots (which of p1 / p2 / p3 carry a
# table), idx, xact, xoff / woff / yoff / ooff (element offset of the base inside its NaN-filled buffer: 2 = 4-byte but not
# 16-byte aligned, 1 = an odd element), nd (*n_dev; None: null pointer), ints, far.
# ---------------------------------------------------------------------------------------------
def _c(entry, N, K, M, act=0, bias=True, **kw):
    c = dict(entry=entry, N=N, K=K, M=M, act=act, bias=bias, slots=(), idx="rand", xact=0, xoff=0, woff=0, yoff=0, ooff=0, nd=None,
             ints=False, far=False)
    assert set(kw) <= set(c), kw
    c.update(kw)
    return c


PLAIN_CASES = {
    # the 15 (kp, nt) forms; N walks {1, 31, 32, 33, 63, 64, 65, 97, 200}: one row, one short of a 32-row half, a half, a half and
    # one row, one short of a tile, a tile, a tile and one row, a tile and a half and one row, three tiles and an 8-row rest;
    # act rotates 0 / 1 / 2; K and M sit on both edges of every padded width
    "p64_1_k4_m1": _c("act", 1, 4, 1, 0, ooff=1, woff=2),        # the smallest layer there is; the output at an odd element
    "p64_2_k62_m33": _c("act", 31, 62, 33, 1, ooff=1),           # K = 62 with a bias: one dword short of the padded row; odd rows at an odd base
    "p64_4": _c("act", 32, 64, 66, 2, bias=False),
    "p64_5_k4": _c("act", 33, 4, 130, 0),                         # five column tiles on two dwords of input
    "p128_1_k66": _c("act", 63, 66, 32, 1, bias=False, woff=2),   # K = 66: the first shape of the 128-wide row
    "p128_2": _c("act", 64, 128, 64, 2),
    "p128_4_k66": _c("act", 65, 66, 128, 0, bias=False),
    "p128_5": _c("act", 97, 128, 160, 1),
    "p160_1_k130_m1": _c("act", 200, 130, 1, 2),                  # KP = 160: the 4-wave map with its 16-dword rest
    "p160_2": _c("act", 1, 160, 64, 0, bias=False),
    "p160_4_k130": _c("act", 33, 130, 66, 1),
    "p160_5": _c("act", 65, 160, 130, 2),                         # the widest layer: M > 128 needs K <= 160
    "p256_1_k162": _c("act", 31, 162, 32, 2),
    "p256_2_m33": _c("act", 97, 256, 33, 1, bias=False),
    "p256_4_k162": _c("act", 200, 162, 128, 0),
    "in_x4": _c("in", 63, 62, 64, 0, xoff=2, woff=2),             # mdl_linear_act_in without a staging: x at a 4-byte base
    "ints200": _c("act", 200, 256, 128, 1, ints=True),            # the longest sum, exact
    # 512 * 64 + 1 rows: workgroup 0 takes a second tile of ONE row behind the grid cap and prefetches it; integer inputs: bit-equal
    "cap512": _c("act", 512 * 64 + 1, 34, 34, 0, ints=True),
}

GATHER_CASES = {
    # every G with every kp and with every nt in {1, 2, 4} (a pairwise cover); which of p1 / p2 / p3 are null varies
    "g1_64_1": _c("gather", 1, 62, 32, 1, slots=(0,)),
    "g1_128_2": _c("gather", 33, 66, 64, 2, bias=False, slots=(1,), idx="equal"),
    "g1_160_4": _c("gather", 65, 160, 66, 0, slots=(2,), idx="last"),
    "g1_256_1_m1": _c("gather", 97, 162, 1, 2, slots=(0,)),
    "g2_64_2_k4": _c("gather", 200, 4, 33, 2, slots=(0, 1)),
    "g2_128_4": _c("gather", 31, 128, 128, 1, bias=False, slots=(0, 2)),
    "g2_160_1": _c("gather", 64, 130, 32, 1, slots=(1, 2), idx="equal"),
    "g2_256_2_k162": _c("gather", 33, 162, 64, 0, slots=(0, 1)),
    "g3_64_4": _c("gather", 63, 64, 128, 0, slots=(0, 1, 2)),
    "g3_128_1": _c("gather", 1, 128, 32, 1, bias=False, slots=(0, 1, 2)),
    "g3_160_2": _c("gather", 32, 160, 34, 2, slots=(0, 1, 2), idx="last"),
    "g3_256_4": _c("gather", 200, 256, 66, 1, slots=(0, 1, 2)),
    "g_ints": _c("gather", 97, 66, 66, 1, slots=(0, 2), ints=True),
}

XACT_CASES = {
    # XACT 1 / 2 with every kp and every nt (pairwise); y post-relu with exact zeros (1) or post-ssp (2)
    "x1_64_5": _c("in", 65, 62, 160, 0, bias=False, xact=1, xoff=2),
    "x1_128_1": _c("in", 33, 128, 32, 1, xact=1, yoff=2),          # y at a 4-byte base, x at a 16-byte one
    "x1_160_2": _c("in", 200, 130, 64, 2, xact=1),
    "x1_256_4": _c("in", 97, 256, 128, 0, xact=1, xoff=2, yoff=2, woff=2),
    "x2_64_2": _c("in", 31, 64, 34, 0, bias=False, xact=2),
    "x2_128_4": _c("in", 64, 66, 66, 1, xact=2, xoff=2),
    "x2_160_5": _c("in", 1, 160, 130, 0, bias=False, xact=2),
    "x2_256_1": _c("in", 200, 162, 32, 2, xact=2, yoff=2),
}

STATS_CASES = {
    # the 15 statistics forms; n_dev null, = N, < N inside the last tile, < N by more than a tile, > N, 0
    "s64_2_k4_m34": _c("stats", 200, 4, 34, 1),
    "s64_4": _c("stats", 97, 62, 66, 0, nd=97),
    "s64_5_m160": _c("stats", 97, 64, 160, 1, bias=False, nd=90),             # the last tile counts 26 of its 33 rows
    "s128_2": _c("stats", 200, 66, 64, 2, nd=100),                            # the last two tiles count nothing
    "s128_4": _c("stats", 63, 128, 128, 1, nd=1000),
    "s128_5": _c("stats", 33, 66, 130, 0, nd=0),                              # n_true = 1
    "s160_2_many": _c("stats", 1089, 160, 34, 1),                             # 18 workgroups: replicas 0 and 1 are added to twice
    "s160_4_far": _c("stats", 200, 130, 66, 1, far=True),                     # a column at 40 +- 0.1: the shift keeps its variance
    "s160_5_k160_m160": _c("stats", 64, 160, 160, 2, bias=False, nd=64),
    "sg64_2": _c("stats", 65, 62, 34, 1, slots=(0, 1)),
    "sg64_4_k4": _c("stats", 200, 4, 128, 1, bias=False, slots=(0, 2), nd=150),
    "sg128_2": _c("stats", 1, 128, 64, 0, slots=(1, 2)),                      # one row: the sums about it are zero
    "sg128_4": _c("stats", 97, 66, 66, 2, slots=(0, 1), nd=97),
    "sg160_2": _c("stats", 33, 130, 64, 1, slots=(0, 1), nd=0, idx="last"),
    "sg160_4_far": _c("stats", 200, 160, 128, 1, slots=(0, 2), far=True),
}

WIDE_CASES = {
    "w64_1blk_192": _c("wide", 448, 62, 192, 0, bias=False),                  # 7 chunks: the plain tile map; one full block
    "w128_2blk_1": _c("wide", 449, 128, 193, 0, bias=False),                  # 8 chunks: the XCD map; a last block of ONE column; odd rows
    "w160_4blk_191": _c("wide", 65, 160, 767, 0, bias=False),                 # 4 blocks, the last 191 wide; odd row stride
    "w64_rounds": _c("wide", 4097, 4, 193, 0, bias=False),                    # 64 chunks and a 65th tile: a second round on chunk 0
    "w160_xcd_4blk": _c("wide", 1024, 130, 768, 0, bias=False),               # 16 chunks x 4 blocks through the XCD map
    "w_ints": _c("wide", 513, 34, 385, 0, bias=False, ints=True),             # 9 chunks (plain), 3 blocks, exact
}
CASES = {**PLAIN_CASES, **GATHER_CASES, **XACT_CASES, **STATS_CASES, **WIDE_CASES}


def case_route(c, x_mod16=None, w_mod4=None, out_mod2=0, y_mod4=None):
    """the route of a case; the GPU test passes the alignments of the pointers it actually hands over"""
    x_mod16 = (2 * c["xoff"]) % 16 if x_mod16 is None else x_mod16
    w_mod4 = (2 * c["woff"]) % 4 if w_mod4 is None else w_mod4
    y_mod4 = (2 * c["yoff"]) % 4 if y_mod4 is None else y_mod4
    if c["entry"] == "wide":
        return wide_route(c["N"], c["K"], c["M"], x_mod16=x_mod16, w_mod4=w_mod4, out_mod2=out_mod2)
    return lin_route(c["entry"], c["N"], c["K"], c["M"], len(c["slots"]), c["xact"], c["entry"] == "stats", act=c["act"],
                     x_mod16=x_mod16, w_mod4=w_mod4, out_mod2=out_mod2, y_mod4=y_mod4)


@functools.lru_cache(maxsize=None)
def case(name):
    """dict(spec, inputs, ref, model, route) of a named case; shared, read-only"""
    c = CASES[name]
    i = make_inputs(c, 900 + sorted(CASES).index(name))
    return dict(spec=c, inputs=i, ref=reference64(i), model=model(i), route=case_route(c))


def mutated(name, mutation):
    return model(case(name)["inputs"], mutation=mutation)


def judge(got, c):
    """dict(ratio, inside, single, equal, ssp_units) of an output `got` [N, M] of case c"""
    i = c["inputs"]
    rep = dict(ratio=row_ratio(got, c["model"]["out"], c["ref"]["out"]), equal=float((got == c["model"]["out"]).double().mean()))
    if c["spec"]["xact"] != 2:
        rep.update(interval_report(got, i))
    return rep


def stat_ratios(sh, S0, S1, c):
    """row_ratio of mean = sh + S0 / n and var = S1 / n - (S0 / n)^2, formed in fp64 from the kernel's numbers"""
    n = n_true_of(c["spec"])
    mean, var = sh.double() + S0.double() / n, S1.double() / n - (S0.double() / n) ** 2
    return dict(mean=row_ratio(mean, c["model"]["mean"], c["ref"]["mean"]), var=row_ratio(var, c["model"]["var"], c["ref"]["var"]))


# ---------------------------------------------------------------------------------------------
# layer level: ops.linear_act / linear_gather_act / linear_relu_bn / matmul_wide on fp32 master weights
# ---------------------------------------------------------------------------------------------
LAYER_N = 130
# name -> (op, N, K, M, act, tables, deterministic, the launches expected: (entry point, K, M, tables))
LAYER_CASES = {
    "act_relu": ("linear_act", 130, 64, 50, "relu", 0, False, [("mdl_linear_act", 64, 50, 0)]),
    "act_ssp": ("linear_act", 130, 130, 66, "ssp", 0, False, [("mdl_linear_act", 130, 66, 0)]),
    "act_none": ("linear_act", 130, 62, 33, None, 0, False, [("mdl_linear_act", 62, 33, 0)]),
    "gather_1": ("linear_gather_act", 130, 64, 64, "relu", 1, False, [("mdl_linear_gather_act", 64, 64, 1)]),
    "gather_2": ("linear_gather_act", 130, 66, 100, None, 2, False, [("mdl_linear_gather_act", 66, 100, 2)]),
    "gather_3": ("linear_gather_act", 130, 160, 32, "relu", 3, False, [("mdl_linear_gather_act", 160, 32, 3)]),
    "bn_0": ("linear_relu_bn", 130, 64, 64, "relu", 0, False, [("mdl_linear_act_stats", 64, 64, 0)]),
    "bn_2": ("linear_relu_bn", 130, 100, 36, "relu", 2, False, [("mdl_linear_act_stats", 100, 36, 2)]),
    "bn_1": ("linear_relu_bn", 130, 64, 64, "relu", 1, False, [("mdl_linear_gather_act", 64, 64, 1), ("mdl_bn_stats_n", 0, 64, 0)]),
    "bn_3": ("linear_relu_bn", 130, 34, 128, "relu", 3, False, [("mdl_linear_gather_act", 34, 128, 3), ("mdl_bn_stats_n", 0, 128, 0)]),
    "bn_0_det": ("linear_relu_bn", 130, 64, 64, "relu", 0, True, [("mdl_linear_act", 64, 64, 0), ("mdl_bn_stats_n", 0, 64, 0)]),
    "bn_2_det": ("linear_relu_bn", 130, 100, 36, "relu", 2, True, [("mdl_linear_gather_act", 100, 36, 2), ("mdl_bn_stats_n", 0, 36, 0)]),
    # ops.matmul_wide's smallest admitted shape (ops.py: 1024 rows, 640 columns): 16 chunks, so the XCD map is taken
    "wide": ("matmul_wide", 1024, 34, 641, None, 0, False, [("mdl_linear_wide", 34, 641, 0)]),
}
# the dX route the backward suite does not reach: M = 20 < 34 keeps the one-pass backward away, so dW / db come from the TN GEMM
# with the activation staging and dX from mdl_linear_act_in — a forward product with kernel K = 20 and kernel M = 64
DX_CASES = {"dx_relu": ("relu", 1), "dx_ssp": ("ssp", 2)}
DX_M, DX_K = 20, 64


def layer_inputs(name):
    op, N, K, M, act, tables, det, calls = LAYER_CASES[name]
    gen = torch.Generator().manual_seed(1300 + sorted(LAYER_CASES).index(name))
    rnd = lambda *s: torch.randn(*s, generator=gen)
    i = dict(x=bfr(rnd(N, K)), w=bfr(rnd(M, K) / K ** 0.5), b=None if op == "matmul_wide" else bfr(rnd(M) * 0.5),
             tables=[bfr(rnd(TABLE_ROWS, M) * 0.5) for _ in range(tables)],
             idx=[torch.randint(0, TABLE_ROWS, (N,), generator=gen, dtype=torch.int32) for _ in range(tables)])
    i["spec"] = _c("gather", N, K, M, {None: 0, "relu": 1, "ssp": 2}[act], bias=i["b"] is not None, slots=tuple(range(tables)))
    i.update(g=None, y=None)
    return i


@functools.lru_cache(maxsize=None)
def layer_case(name):
    i = layer_inputs(name)
    return dict(inputs=i, spec=i["spec"], ref=reference64(i), model=model(i), calls=LAYER_CASES[name][7])


def batchnorm64(y, gamma, beta, eps, momentum):
    """training-mode BatchNorm1d of the rows y in fp64: (z, running_mean, running_var) from running statistics (0, 1)"""
    y = y.double()
    n = y.shape[0]
    mean, var = y.mean(0), y.var(0, unbiased=False)
    z = (y - mean) / torch.sqrt(var + eps) * gamma.double() + beta.double()
    return z, momentum * mean, (1 - momentum) + momentum * var * n / (n - 1)


@functools.lru_cache(maxsize=None)
def dx_layer(name):
    """x [N, K], w [M, K], b [M], gout [N, M] of the layer whose input gradient is wanted"""
    act, code = DX_CASES[name]
    gen = torch.Generator().manual_seed(1400 + code)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    return dict(x=bfr(rnd(LAYER_N, DX_K)), w=bfr(rnd(DX_M, DX_K) / DX_K ** 0.5), b=bfr(rnd(DX_M) * 0.5), gout=bfr(rnd(LAYER_N, DX_M)),
                act=act, code=code)


def dx_from(name, y):
    """dX = (gout .* act'(y)) W from the output y the layer SAVED (its own forward's, bit for bit): an "in" case with kernel
    K = M and kernel M = K, its weight W^T"""
    L = dx_layer(name)
    c = _c("in", LAYER_N, DX_M, DX_K, 0, bias=False, xact=L["code"])
    i = dict(spec=c, x=None, g=L["gout"], y=y, w=L["w"].t().contiguous(), b=None, tables=[], idx=[])
    return dict(inputs=i, spec=c, ref=reference64(i), model=model(i))
