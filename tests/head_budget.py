"""Error budget of the readout head and the step tail against an fp64 reference (helper module of test_head_budget_host.py and
test_gpu_head_budget.py; no test lives here).  It follows tests/stream_budget.py: the yardstick is a ROUNDING MODEL, the same
arithmetic in plain fp32 torch on the CPU, rounded to bf16 exactly where the kernel stores bf16; a kernel output may stand
ALLOWED[tensor] times the model's own distance from fp64, per row, and a structural bug stands far over it (MUTATIONS).

  csrc/mlp.hip    the fused post-FC head: mdl_mlp_head_fwd, mdl_mlp_head_bwd                              MLP_CASES
  csrc/gru.hip    the gate arithmetic of one GRU step: mdl_gru_gates_fwd, mdl_gru_gates_bwd               GRU_CASES
  csrc/loss.hip   mean L1 / MSE loss and its gradient: mdl_loss_fwd_bwd, mdl_loss_fwd_bwd_rows            LOSS_CASES

Measures:
  tight    ratio(got, model, ref64) <= ALLOWED[tensor]: row_ratio of cgconv_budget.py, rows = data rows for y / h / dx / h_out /
           dgi / dgh / dh and output channels for dW; db and the loss value are one row (vec_ratio of stream_budget.py: the model's
           error floored at half an ulp of fp32).  dW carries the same floor per row (a one-row dW of a 1-column head is a vector).
           So that one bf16 tie or one ReLU flip does not drown the measure, the forward is judged LAYER BY LAYER (layer l of the
           kernel against model and fp64 applied to the kernel's own stored output of layer l - 1) and the backward ON GIVEN HIDDEN
           OUTPUTS (model and fp64 evaluated on the h the kernel was handed).
  derived  nothing in it is measured.
             pre-activation   within (K + 1) 2^-24 (sum|x_k w_k| + |b|) of fp64: the stored bf16 value is a bf16 rounding of a point
                              of that interval, after the ReLU (mlp_interval; `single` = share of intervals that admit ONE value)
             dW, db, top layer  within N 2^-24 sum|term| of the fp64 sum of the terms the kernel adds (gy as the kernel rounds it,
                              times the stored input).  The dZ of the lower layers never leaves the kernel: their dW and db stand
                              under the tight measure alone, and under equality on integer data.
             loss             within (n + 2) 2^-24 sum|term| / n of the fp64 mean of the fp32 terms
             loss gradients   L1: +-fl(1/n), 0 at a tie; MSE: fl(fl(2 d) fl(1/n)), d = fl(p - y): bit for bit
           dx also has to AGREE with the model: at least AGREE_MIN of its elements bit-equal.  An element differs only where the
           order of an fp32 sum moves a value across a bf16 rounding boundary (65 2^-24 of the magnitude against a spacing of 2^-8:
           a per-mille of the elements, and a flipped dZ element moves a tenth of its row's 64) - a kernel that skips the rounding
           of dZ moves every dIn by half a bf16 step and agrees in about two elements of three.  0.9 lies between the two.
  exact    integer data (inputs, biases, gy in {-1, 0, 1}; at most two +-1 in every weight row and column): every stored bf16
           is an integer <= 256, every fp32 partial sum below 2^24, the result the same in any order: equality with the model.

The table of measured ratios stands in front of ALLOWED below.
"""
import functools
import math

import torch

from cgconv_budget import bfr, fmt, row_ratio, row_rms  # noqa: F401  (re-exported for the tests)
from linear_budget import bf_step
from stream_budget import vec_ratio  # noqa: F401

PAD_ROWS = 70                                    # NaN rows behind every operand
GUARD = 256                                      # bytes behind every output in the arenas of the GPU test
U = 2.0 ** -24                                   # unit roundoff of fp32
AGREE_MIN = 0.9                                  # share of dx elements bit-equal to the model (see above)
MLP_TENSORS = ("y", "h", "dx", "dw", "db")
GRU_TENSORS = ("h_out", "dgi", "dgh", "dh")
OK, E_ARG, E_UNSUPP = 0, -1, -2                  # mdlStatus (include/mdl_hip.h)

# Permitted ratio per tensor: twice the largest value measured on the MI355X over every case of test_gpu_head_budget.py and two
# runs, rounded up to one decimal, never below 2 and never above 5 (the rule of cgconv_budget.py and stream_budget.py).
# Measured on the MI355X (the [budget] lines of one run; `largest` is over every run made): per case the route and the ratios; `single`
# = per layer the share of elements whose derived interval admits ONE bf16 value (every element of every case lay inside its
# interval); bound_dw / bound_db = the largest error of the top layer's sums as a fraction of the derived bound; `agree` = the share
# of dx elements bit-equal to the model; for the loss, `bound` = the error as a fraction of its derived bound.  The backward lines
# hold the larger of two launches.
#   ref_batch          fwd grid 2 trips 1 | bwd grid 2 trips 1 gy odd   h 1.000  y 1.000   single 0.983 0.985 0.989 1.000
#   ref_batch          bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.005  bound_db 0.000   agree 1.0
#   ref_batch          bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.005  bound_db 0.000   agree 1.0
#   ref_batch_f32io    fwd grid 2 trips 1 | bwd grid 2 trips 1 gy f32   h 1.000  y 1.000   single 0.982 0.988 0.988 0.990
#   ref_batch_f32io    bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.004  bound_db 0.000   agree 1.0
#   ref_batch_f32io    bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.004  bound_db 0.000   agree 1.0
#   n1                 fwd grid 1 trips 1 | bwd grid 1 trips 1 gy even   h 1.000  y 1.000   single 0.969 1.000
#   n1                 bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   n1                 bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   n63                fwd grid 1 trips 1 | bwd grid 1 trips 1 gy even   h 1.000  y 1.000   single 0.982 1.000
#   n63                bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.009  bound_db 0.000   agree 1.0
#   n63                bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.009  bound_db 0.000   agree 1.0
#   n64                fwd grid 1 trips 1 | bwd grid 1 trips 1 gy even   h 1.000  y 1.000   single 0.980 1.000
#   n64                bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.009  bound_db 0.000   agree 1.0
#   n64                bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.009  bound_db 0.000   agree 1.0
#   n65                fwd grid 2 trips 1 | bwd grid 2 trips 1 gy even   h 1.000  y 1.000   single 0.984 0.985
#   n65                bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.009  bound_db 0.000   agree 1.0
#   n65                bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.009  bound_db 0.000   agree 1.0
#   n129               fwd grid 3 trips 1 | bwd grid 3 trips 1 gy even   h 1.000  y 1.000   single 0.980 0.981
#   n129               bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.003  bound_db 0.000   agree 1.0
#   n129               bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.003  bound_db 0.000   agree 1.0
#   narrow             fwd grid 5 trips 1 | bwd grid 5 trips 1 gy even   h 1.000  y 1.000   single 0.997 0.988 0.972
#   narrow             bwd on model h dx 1.000  dw 1.144  db 1.000  bound_dw 0.002  bound_db 0.000   agree 1.0
#   narrow             bwd on own h   dx 1.000  dw 1.181  db 1.000  bound_dw 0.002  bound_db 0.000   agree 1.0
#   tiny               fwd grid 3 trips 1 | bwd grid 3 trips 1 gy odd   h 1.000  y 1.000   single 0.992 0.977
#   tiny               bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.001  bound_db 0.000   agree 1.0
#   tiny               bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.001  bound_db 0.000   agree 1.0
#   ragged_widths      fwd grid 4 trips 1 | bwd grid 4 trips 1 gy odd   h 1.000  y 1.000   single 0.985 0.994 0.973
#   ragged_widths      bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.003  bound_db 0.000   agree 1.0
#   ragged_widths      bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.003  bound_db 0.000   agree 1.0
#   one_layer_40       fwd grid 5 trips 1 | bwd grid 5 trips 1 gy even   y 1.000   single 0.965
#   one_layer_40       bwd on model h dx 1.000  dw 0.902  db 0.259  bound_dw 0.002  bound_db 0.000   agree 1.0
#   one_layer_40       bwd on own h   dx 1.000  dw 1.033  db 0.259  bound_dw 0.002  bound_db 0.000   agree 1.0
#   one_layer_1        fwd grid 5 trips 1 | bwd grid 5 trips 1 gy odd   y 1.000   single 0.980
#   one_layer_1        bwd on model h dx 1.000  dw 0.591  db 0.000  bound_dw 0.001  bound_db 0.000   agree 1.0
#   one_layer_1        bwd on own h   dx 1.000  dw 0.556  db 0.000  bound_dw 0.001  bound_db 0.000   agree 1.0
#   four_layers        fwd grid 5 trips 1 | bwd grid 5 trips 1 gy even   h 1.000  y 1.000   single 0.982 0.988 0.987 0.975
#   four_layers        bwd on model h dx 1.000  dw 1.279  db 1.000  bound_dw 0.004  bound_db 0.000   agree 1.0
#   four_layers        bwd on own h   dx 1.000  dw 1.279  db 1.000  bound_dw 0.004  bound_db 0.000   agree 1.0
#   no_bias_mix        fwd grid 2 trips 1 | bwd grid 2 trips 1 gy odd   h 1.000  y 1.000   single 0.981 0.985 0.989 1.000
#   no_bias_mix        bwd on model h dw 1.000  db 1.000  bound_dw 0.003   agree None
#   no_bias_mix        bwd on own h   dw 1.000  db 1.000  bound_dw 0.003   agree None
#   cancel             fwd grid 5 trips 1 | bwd grid 5 trips 1 gy odd   h 1.000  y 1.000   single 0.499 0.999 0.988
#   cancel             bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.001  bound_db 0.000   agree 1.0
#   cancel             bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.001  bound_db 0.000   agree 1.0
#   dead               fwd grid 5 trips 1 | bwd grid 5 trips 1 gy odd   h 0.000  y 0.000   single 1.000 1.000 1.000
#   dead               bwd on model h dx 0.000  dw 0.000  db 0.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   dead               bwd on own h   dx 0.000  dw 0.000  db 0.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   det                fwd grid 5 trips 1 | bwd grid 1 trips 5 gy odd   h 1.000  y 1.000   single 0.983 0.988 0.957
#   det                bwd on model h dx 1.000  dw 1.000  db 1.000  bound_dw 0.002  bound_db 0.000   agree 1.0
#   det                bwd on own h   dx 1.000  dw 1.000  db 1.000  bound_dw 0.002  bound_db 0.000   agree 1.0
#   trip2_fwd_int      fwd grid 512 trips 2 | bwd grid 256 trips 3 gy odd   h 0.000  y 0.000   single 0.778 0.863 0.867 1.000
#   trip2_fwd_int      bwd on model h dx 0.000  dw 0.000  db 0.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   trip2_fwd_int      bwd on own h   dx 0.000  dw 0.000  db 0.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   trip2_bwd_int      fwd grid 258 trips 1 | bwd grid 256 trips 2 gy odd   h 0.000  y 0.000   single 0.778 0.861 0.894 1.000
#   trip2_bwd_int      bwd on model h dx 0.000  dw 0.000  db 0.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   trip2_bwd_int      bwd on own h   dx 0.000  dw 0.000  db 0.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   trip2_bwd_int_det  fwd grid 258 trips 1 | bwd grid 1 trips 258 gy odd   h 0.000  y 0.000   single 0.777 0.859 0.851 0.216
#   trip2_bwd_int_det  bwd on model h dx 0.000  dw 0.000  db 0.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   trip2_bwd_int_det  bwd on own h   dx 0.000  dw 0.000  db 0.000  bound_dw 0.000  bound_db 0.000   agree 1.0
#   v4_100_f           fwd W4 grid 26 trips 1 | bwd W4 grid 26 trips 1   h_out 1.312  dgi 1.345  dgh 1.250  dh 1.074
#   v4_4_f             fwd W4 grid 1 trips 1 | bwd W4 grid 1 trips 1   h_out 1.022  dgi 1.000  dgh 1.000  dh 1.000
#   s_7_f              fwd W1 grid 1 trips 1 | bwd W1 grid 1 trips 1   h_out 0.954  dgi 1.034  dgh 1.012  dh 1.000
#   s_30_f             fwd W1 grid 16 trips 1 | bwd W1 grid 16 trips 1   h_out 1.530  dgi 1.445  dgh 1.391  dh 1.193
#   trip2_v4_f         fwd W4 grid 2048 trips 2 | bwd W4 grid 2048 trips 2   h_out 1.223  dgi 1.227  dgh 1.303  dh 1.209
#   trip2_s_f          fwd W1 grid 2048 trips 2 | bwd W1 grid 2048 trips 2   h_out 1.670  dgi 2.102  dgh 2.329  dh 1.787
#   saturated_f        fwd W4 grid 9 trips 1 | bwd W4 grid 9 trips 1   h_out 1.188  dgi 0.508  dgh 0.528  dh 1.046
#   zero_state_f       fwd W4 grid 3 trips 1 | bwd W4 grid 3 trips 1   h_out 1.132  dgi 1.217  dgh 1.366  dh 1.155
#   v4_100_b           fwd W4 grid 26 trips 1 | bwd W4 grid 26 trips 1   h_out 1.237  dgi 1.000  dgh 1.000  dh 1.185
#   v4_4_b             fwd W4 grid 1 trips 1 | bwd W4 grid 1 trips 1   h_out 0.684  dgi 1.000  dgh 1.000  dh 1.000
#   s_7_b              fwd W1 grid 1 trips 1 | bwd W1 grid 1 trips 1   h_out 1.261  dgi 1.000  dgh 1.000  dh 1.000
#   s_30_b             fwd W1 grid 16 trips 1 | bwd W1 grid 16 trips 1   h_out 1.846  dgi 1.000  dgh 1.000  dh 1.030
#   trip2_v4_b         fwd W4 grid 2048 trips 2 | bwd W4 grid 2048 trips 2   h_out 1.172  dgi 1.000  dgh 1.000  dh 1.205
#   trip2_s_b          fwd W1 grid 2048 trips 2 | bwd W1 grid 2048 trips 2   h_out 1.545  dgi 1.000  dgh 1.000  dh 1.555
#   saturated_b        fwd W4 grid 9 trips 1 | bwd W4 grid 9 trips 1   h_out 1.428  dgi 1.000  dgh 1.000  dh 1.330
#   zero_state_b       fwd W4 grid 3 trips 1 | bwd W4 grid 3 trips 1   h_out 1.049  dgi 1.000  dgh 1.000  dh 1.113
#   misaligned_gi_b    fwd W1 grid 65 trips 1 | bwd W1 grid 65 trips 1   h_out 1.221  dgi 1.000  dgh 1.000  dh 1.254
#   misaligned_h_f     fwd W1 grid 65 trips 1 | bwd W1 grid 65 trips 1   h_out 1.274  dgi 1.274  dgh 1.256  dh 1.174
#   misaligned_glp_b   fwd W4 grid 17 trips 1 | bwd W1 grid 65 trips 1   h_out 1.320  dgi 1.000  dgh 1.000  dh 1.292
#   g_h_only_b         fwd W4 grid 9 trips 1 | bwd W4 grid 9 trips 1   h_out 1.118  dgi 1.000  dgh 1.000  dh 1.106
#   g_lp_only_b        fwd W4 grid 9 trips 1 | bwd W4 grid 9 trips 1   h_out 1.188  dgi 1.000  dgh 1.000  dh 1.111
#   no_out_lp_b        fwd W4 grid 9 trips 1 | bwd W4 grid 9 trips 1   h_out 1.296  dgi 1.000  dgh 1.000  dh 1.258
#   n1_l1              loss 0.000  bound 0.000
#   n1_mse             loss 1.000  bound 0.000
#   n63_l1             loss 1.000  bound 0.023
#   n63_mse            loss 0.083  bound 0.000
#   n64_l1             loss 0.685  bound 0.010
#   n64_mse            loss 0.764  bound 0.008
#   n65_l1             loss 0.225  bound 0.003
#   n65_mse            loss 1.045  bound 0.022
#   n1023_l1           loss 0.361  bound 0.000
#   n1023_mse          loss 0.649  bound 0.001
#   n1024_l1           loss 0.055  bound 0.000
#   n1024_mse          loss 0.374  bound 0.000
#   n1025_l1           loss 0.581  bound 0.001
#   n1025_mse          loss 0.298  bound 0.000
#   n8193_l1           loss 0.844  bound 0.000
#   n8193_mse          loss 0.653  bound 0.000
#   rows_1_l1          loss 1.637  bound 0.008
#   rows_1_mse         loss 0.397  bound 0.002
#   rows_1024_l1       loss 0.826  bound 0.004
#   rows_1024_mse      loss 1.000  bound 0.008
#   rows_3000_l1       loss 0.262  bound 0.002
#   rows_3000_mse      loss 0.954  bound 0.005
#   ties_l1            loss 0.275  bound 0.000
#   ties_mse           loss 0.199  bound 0.000
#   int_l1             loss 0.828  bound 0.000
#   int_mse            loss 0.938  bound 0.000
#   int_rows_l1        loss 0.068  bound 0.000
#   int_rows_mse       loss 1.000  bound 0.000
#   aligned_l1         loss 0.030  bound 0.000
#   aligned_mse        loss 0.099  bound 0.000
# largest: y 1.000, h 1.000, dx 1.000, db 1.000 (the rounding to bf16 dominates both sides; fp32 db: vec_ratio at its floor);
# dw 1.334 (four_layers, 1.279 - 1.334 over two runs; 1.14 - 1.20 on narrow: the atomics' order differs from launch to launch); h_out 1.846 (s_30_b); dgi 2.102,
# dgh 2.329, dh 1.787 (trip2_s_f: the largest of 10487 rows); loss 1.637 (rows_1_l1).  Of the derived bounds: top-layer dW 0.009
# (n63 - n65), db 0.000 (a sum of a few hundred bf16 values is exact in fp32), loss 0.023 (n63_l1).  single-valued intervals: 0.96 -
# 1.00 of the elements of the random cases, 0.499 in layer 0 of `cancel` (what the case is for), 0.78 - 0.89 in the integer cases (an
# exact 0 with a non-zero magnitude admits 0 and the smallest positive value).
# Notes.
#   0.000: model and kernel both exact (integer data, `dead`).  1.000: the rounding to bf16 dominates both sides.
#   dx agreed with the model in EVERY element of every case, and the kernel's own hidden outputs were the model's in every case:
#   the second backward of each case ran on the same bits as the first.
#   The device's 1.0f / (float)n is correctly rounded: every L1 and MSE gradient was bit-equal to fl(1/n) arithmetic.
#   saturated (fp32): dgi 0.508, dgh 0.528 with the floor of 2^-22 |g (1 - z)|; without it the quotient is one of two lost accuracies.
#   No kernel or launcher bug came out of these cases.  ops.mlp_head_ok said yes to an input of 0 columns and to a layer of 0 outputs,
#   which mlp_check refuses (MDL_E_UNSUPP): fixed in ops.py, pinned by test_mlp_head_ok_is_true_only_where_the_entry_points_accept.
ALLOWED = {"y": 2.0, "h": 2.0, "dx": 2.0, "dw": 2.7, "db": 2.0, "h_out": 3.7, "dgi": 4.3, "dgh": 4.7, "dh": 3.6, "loss": 3.3}


def cdiv(a, b):
    return -(-a // b)


def _ident(t):
    return t


def f3(r):
    """fmt with three decimals (ALLOWED is formed from these figures)"""
    return "  ".join("%s %.3f" % (k, v) for k, v in r.items())


def ratio(got, model, ref64, floor=None):
    """row_ratio with the model's row error floored (as well) at `floor` [rows]; floor = None IS row_ratio (the host test pins it)"""
    e_got, e_mod = row_rms(got, ref64), row_rms(model, ref64)
    den = torch.clamp(e_mod, min=float(e_mod.median()))
    if floor is not None:
        den = torch.maximum(den, floor.to(den.dtype))
    return float(torch.where(e_got == 0, torch.zeros_like(e_got), e_got / den.clamp(min=1e-300)).max())


def ulp_floor(ref64):
    """per row: half an ulp of fp32 at the reference values"""
    r = ref64.double()
    r = r.view(1, -1) if r.dim() < 2 else r
    return r.mul(U).pow(2).mean(dim=1).sqrt()


# ---------------------------------------------------------------------------------------------
# the dispatches, restated: the kernel choice is made in C and is not observable from Python
# ---------------------------------------------------------------------------------------------
def mlp_route(N, K0, M, f32io, det, direction):
    """(tiles, grid, trips per workgroup, LDS bytes, gy staging) of csrc/mlp.hip:
      tiles  cdiv(N, 64) row tiles
      grid   min(tiles, 512) forward (line 319), min(tiles, 256) backward and 1 under MDL_DETERMINISTIC (lines 353-355)
      LDS    (NL + 2) 64 72 2 forward: the weights and two tiles; (2 NL + 2) 64 72 2 backward: transposed weights, every layer's
             input tile, two dZ tiles
      gy     backward: "f32" under MDL_MLP_F32_IO (mlp_stage_f32), else "odd" (element by element, a 2-byte aligned base is
             enough) for an odd last width, else "even" (dwords); forward: None"""
    assert direction in ("fwd", "bwd") and N >= 1
    NL = len(M)
    tiles = cdiv(N, 64)
    if direction == "fwd":
        grid, lds, gy = min(tiles, 512), (NL + 2) * 64 * 72 * 2, None
    else:
        grid, lds = (1 if det else min(tiles, 256)), (2 * NL + 2) * 64 * 72 * 2
        gy = "f32" if f32io else ("odd" if M[-1] % 2 else "even")
    return (tiles, grid, cdiv(tiles, grid), lds, gy)


def mlp_accepts(direction, N, K0, M, dtype="bf16", f32io=False, x=0, w=None, h=None, gy=0, dw=None, arrays=True):
    """the return code of mdl_mlp_head_fwd / _bwd, restated in the order the checks run (mlp_check, lines 286-297, and the entry
    points' own MDL_REQUIREs).  Pointers are addresses (None: null); w / h / dw default to aligned non-null entries.
    h: forward the NL outputs, backward the NL - 1 saved hidden outputs."""
    NL = len(M)
    w = [0] * NL if w is None else w
    h = [0] * NL if h is None else h
    dw = [0] * NL if dw is None else dw
    if not (1 <= NL <= 4 and arrays):
        return E_ARG
    if dtype != "bf16":
        return E_UNSUPP
    if not (2 <= K0 <= 64 and K0 % 2 == 0):
        return E_UNSUPP
    for l in range(NL):
        if not (1 <= M[l] <= 64 and (l + 1 == NL or M[l] % 2 == 0)):
            return E_UNSUPP
        if w[l] is None or w[l] % 4:
            return E_ARG
    if not (N >= 0 and (N == 0 or (x is not None and x % 4 == 0))):
        return E_ARG
    if direction == "fwd":
        if N and any(h[l] is None for l in range(NL)):
            return E_ARG
        return OK
    if N and (gy is None or gy % (2 if (M[-1] % 2 and not f32io) else 4)):
        return E_ARG
    for l in range(NL):
        if N and dw[l] is None:
            return E_ARG
        if N and l + 1 < NL and (h[l] is None or h[l] % 4):
            return E_ARG
    return OK


def head_ok(dtype, dim, contiguous, N, K0, x_addr, widths, in_features, requires_grad, act="relu"):
    """ops.mlp_head_ok restated on plain numbers (ops.py: the fused head takes bf16 device rows, 1..4 layers of width <= 64, hidden
    widths even, ReLU between)"""
    if not (act == "relu" and dtype == "bf16" and dim == 2 and contiguous and 1 <= len(widths) <= 4 and N >= 1 and 2 <= K0 <= 64
            and K0 % 2 == 0 and x_addr % 4 == 0):
        return False
    k = K0
    for j, m in enumerate(widths):
        if in_features[j] != k or not 1 <= m <= 64 or (j + 1 < len(widths) and m % 2) or not requires_grad[j]:
            return False
        k = m
    return True


def gru_route(N, C, dtype, alignments):
    """(W, grid, trips) of csrc/gru.hip.  alignments = dict(lp = addresses of the pointers of the compute dtype (fwd: gi, gh,
    out_lp; bwd: gi, gh, g_lp, dgi, dgh), f32 = addresses of the fp32 ones (fwd: h, h_out; bwd: h, dh, g_h)); None is a null
    optional pointer and counts as aligned.
      gru_vec_ok (lines 100-106)  C % 4 == 0 and every lp pointer on min(4 sizeof(T), 16) bytes: 8 for bf16, 16 for fp32
      f32ok (lines 118, 143)      every fp32 pointer on 16 bytes
      W = 4 if both, else 1; grid = cdiv(N C / W, 256) in [1, 2048] (gru_grid); trips of the grid-stride loop"""
    assert dtype in ("bf16", "f32") and N >= 1 and 1 <= C <= 65536
    al = 8 if dtype == "bf16" else 16
    vec_ok = C % 4 == 0 and all(p is None or p % al == 0 for p in alignments["lp"])
    f32ok = all(p is None or p % 16 == 0 for p in alignments["f32"])
    W = 4 if (vec_ok and f32ok) else 1
    total = N * (C // W)
    grid = min(max(cdiv(total, 256), 1), 2048)
    return (W, grid, cdiv(total, grid * 256))


# ---------------------------------------------------------------------------------------------
# MLP head: cases
# ---------------------------------------------------------------------------------------------
def _mlp(N, K0, M, **kw):
    c = dict(N=N, K0=K0, M=tuple(M), f32io=False, det=False, kind="randn", nobias=(), dx=True, gy_off=0)
    c.update(kw)
    return c


_W4 = (64, 64, 64, 1)
MLP_CASES = {
    "ref_batch": _mlp(101, 64, _W4), "ref_batch_f32io": _mlp(101, 64, _W4, f32io=True),
    "n1": _mlp(1, 64, (32, 2)), "n63": _mlp(63, 64, (32, 2)), "n64": _mlp(64, 64, (32, 2)), "n65": _mlp(65, 64, (32, 2)),
    "n129": _mlp(129, 64, (32, 2)),
    "narrow": _mlp(257, 16, (64, 64, 8)),
    "tiny": _mlp(130, 2, (2, 1)),
    "ragged_widths": _mlp(200, 50, (34, 62, 3), gy_off=1),            # odd last width, bf16 gy at an address = 2 (mod 4)
    "one_layer_40": _mlp(300, 64, (40,)), "one_layer_1": _mlp(300, 64, (1,)),
    "four_layers": _mlp(300, 64, (64, 64, 64, 64)),                   # the largest LDS footprint both ways
    "no_bias_mix": _mlp(101, 64, _W4, nobias=(1, 3), dx=False),       # b[1], b[3], db[1], db[3] and dx null
    "cancel": _mlp(257, 64, (64, 64, 1), kind="cancel"),
    "dead": _mlp(257, 64, (64, 64, 1), kind="dead"),
    "det": _mlp(300, 64, (64, 64, 1), det=True),
    "trip2_fwd_int": _mlp(512 * 64 + 65, 64, _W4, kind="int"),        # the forward loop's second trip, ragged last tile
    "trip2_bwd_int": _mlp(256 * 64 + 65, 64, _W4, kind="int"),        # the backward loop's second trip: dW carried in registers
    "trip2_bwd_int_det": _mlp(256 * 64 + 65, 64, _W4, kind="int", det=True),      # one workgroup, 258 trips
}


def mlp_case_routes(c):
    return (mlp_route(c["N"], c["K0"], c["M"], c["f32io"], c["det"], "fwd"), mlp_route(c["N"], c["K0"], c["M"], c["f32io"], c["det"], "bwd"))


def mlp_inputs(c, seed):
    """x [N, K0], w[l] [M_l, K_l], b[l] [M_l] or None, gy [N, M_last]: fp32 tensors, exact in bf16 (gy under MDL_MLP_F32_IO: not)"""
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    N, K0, M, kind = c["N"], c["K0"], list(c["M"]), c["kind"]
    Ks = [K0] + M[:-1]
    NL = len(M)
    if kind == "int":
        tri = lambda *s: torch.randint(-1, 2, s, generator=gen).float()
        x, gy, b, w = tri(N, K0), tri(N, M[-1]), [tri(m) for m in M], []
        for m, k in zip(M, Ks):
            assert m <= k                                            # (then every column holds at most two entries as well)
            wl = torch.zeros(m, k)
            sg = torch.randint(0, 2, (m, 2), generator=gen).float() * 2 - 1
            for r in range(m):
                wl[r, r % k], wl[r, (r + 7) % k] = sg[r, 0], sg[r, 1]
            w.append(wl)
    else:
        x = bfr(rnd(N, K0))
        w = [bfr(rnd(m, k) / math.sqrt(k)) for m, k in zip(M, Ks)]
        b = [bfr(0.3 * rnd(m)) for m in M]
        gy = rnd(N, M[-1])
        gy = gy if c["f32io"] else bfr(gy)
        if kind == "cancel":
            # x = [u | -u] and W_0 = [A | a bf16 neighbour of A], b_0 = 0: x W_0^T = u (A - A'), a sum of single bf16 steps of
            # the products - most pre-activations of layer 0 lie within a few bf16 steps of zero, of either sign
            u, A = x[:, :K0 // 2], w[0][:, :K0 // 2]
            x = torch.cat([u, -u], 1)
            w[0] = torch.cat([A, bf_step(A, torch.randint(-1, 2, A.shape, generator=gen).to(torch.int32))], 1)
            b[0] = torch.zeros(M[0])
        if kind == "dead":
            for l in range(NL - 1):
                b[l] = bfr(-(8.0 + rnd(M[l]).abs()))
    b = [None if l in c["nobias"] else b[l] for l in range(NL)]
    return dict(N=N, K0=K0, M=M, Ks=Ks, NL=NL, f32io=c["f32io"], kind=kind, x=x, w=w, b=b, gy=gy, nobias=tuple(c["nobias"]), want_dx=c["dx"])


def mlp_layer(i, l, inp, dt=torch.float32, rounded=True, mutation=None, carry=False):
    """layer l applied to `inp` in `dt`.  fp32 with rounded = True is the MODEL of mlp_head_fwd_kernel: fp32 products and sums on
    the bias read as bf16, the ReLU (all layers but the last), ONE rounding to bf16 (the fp32 output under MDL_MLP_F32_IO holds
    the rounded value).  carry = True returns (stored, handed on): the two differ under a mutation only."""
    NL = i["NL"]
    last = l == NL - 1
    w, a = i["w"][l].to(dt), inp.to(dt)
    if mutation == "drop_kstep" and l == min(1, NL - 1):
        a = a.clone()
        a[:, (cdiv(a.shape[1], 16) - 1) * 16:] = 0
    z = a @ w.t()
    if i["b"][l] is not None and not (mutation == "skip_last_bias" and last):
        z = z + i["b"][l].to(dt)
    if not last or mutation == "relu_last":
        z = torch.relu(z)
    stored = bfr(z) if rounded else z
    on = z if (mutation == "hidden_fp32" and not last) else stored
    if mutation == "dirty_pad_columns" and not last and i["M"][l] < 64:
        on = on + float("nan")                                       # NaN in a column >= M of the tile: NaN x (zero weight) = NaN
    return (stored, on) if carry else stored


def mlp_forward(i, dt=torch.float32, rounded=True, mutation=None):
    """the stored outputs of every layer, chained"""
    out, a = [], i["x"]
    for l in range(i["NL"]):
        s, a = mlp_layer(i, l, a, dt, rounded, mutation, carry=True)
        out.append(s)
    return out


def mlp_backward(i, hs, dt=torch.float32, rounded=True, mutation=None):
    """dict(dx, dw [NL], db [NL]) on the GIVEN hidden outputs hs [NL - 1] in `dt`.  fp32 with rounded = True is the MODEL of
    mlp_head_bwd_kernel: dZ_last = gy (rounded to bf16 under MDL_MLP_F32_IO), dW_l = dZ_l^T in_l and db_l = column sums of dZ_l in
    fp32, dIn_l = dZ_l W_l in fp32, dZ_{l-1} = bf16(dIn_l where h_{l-1} > 0), dx = bf16(dIn_0)."""
    NL, N = i["NL"], i["N"]
    r = bfr if rounded else _ident
    dz = i["gy"].to(dt)
    if i["f32io"] and mutation != "gy_not_rounded":
        dz = r(dz).to(dt)
    keep = torch.ones(N, 1, dtype=dt)
    if mutation == "ragged_rows_missing":
        keep[N // 64 * 64:] = 0
    if mutation == "trip2_rows_missing":
        keep[256 * 64:] = 0
    dzs, dw, db = [None] * NL, [None] * NL, [None] * NL
    dx = None
    for l in range(NL - 1, -1, -1):
        a = (i["x"] if l == 0 else hs[l - 1]).to(dt)
        dzs[l] = dz
        dw[l] = (dz * keep).t() @ a
        if mutation == "nan_rows_included":
            dw[l] = dw[l] + float("nan")
        db[l] = dz.sum(0)
        w = i["w"][l].to(dt)
        din = dz @ (w.t() if (mutation == "w_untransposed" and w.shape[0] == w.shape[1]) else w)
        if l > 0:
            mask = (hs[l - 1] >= 0) if mutation == "mask_ge" else (hs[l - 1] > 0)
            dz = torch.where(mask, din, torch.zeros_like(din))
            dz = dz if mutation == "dz_not_rounded" else r(dz).to(dt)
        elif i["want_dx"]:
            dx = r(din)
    if mutation == "db_wrong_layer":
        for l in range(NL - 1):
            if i["M"][l] == i["M"][l + 1]:
                db[l], db[l + 1] = db[l + 1], db[l]
                break
    db = [None if l in i["nobias"] else db[l] for l in range(NL)]
    return dict(dx=dx, dw=dw, db=db, dz_top=dzs[NL - 1])


def mlp_interval(i, l, inp):
    """(lo, hi, single): the bf16 values between which every stored element of layer l must lie, given its stored input"""
    a, w = inp.double(), i["w"][l].double()
    s, mag = a @ w.t(), a.abs() @ w.abs().t()
    if i["b"][l] is not None:
        s, mag = s + i["b"][l].double(), mag + i["b"][l].double().abs()
    t = i["Ks"][l] + 1
    delta = t * U / (1 - t * U) * mag * (1 + 2.0 ** -30)
    act = _ident if l == i["NL"] - 1 else torch.relu
    lo, hi = bfr(act(s - delta).float()), bfr(act(s + delta).float())
    # (fp64 -> fp32 -> bf16 is a double rounding: widen by the fp32 step so that the interval never loses a value)
    lo, hi = torch.minimum(lo, bfr((act(s - delta) * (1 - 2 * U)).float())), torch.maximum(hi, bfr((act(s + delta) * (1 + 2 * U)).float()))
    lo, hi = torch.minimum(lo, bfr((act(s - delta) * (1 + 2 * U)).float())), torch.maximum(hi, bfr((act(s + delta) * (1 - 2 * U)).float()))
    return lo, hi, float((lo == hi).double().mean())


def _over(fails, name, value, allowed, factor):
    if not value <= factor * allowed:
        fails.append("%s at %.3g x (allowed %.1f)" % (name, value, allowed))


def mlp_judge_fwd(i, layers, factor=1.0):
    """(fails, report) of the stored outputs of every layer, layer by layer on the kernel's own stored input"""
    fails, rep = [], dict(ratios={}, single=[], inside=[])
    NL = i["NL"]
    for l in range(NL):
        got = layers[l]
        key = "y" if l == NL - 1 else "h"
        if not bool(torch.isfinite(got).all()):
            fails.append("%s%d not finite" % (key, l))
            continue
        inp = i["x"] if l == 0 else layers[l - 1]
        mod, ref = mlp_layer(i, l, inp), mlp_layer(i, l, inp, torch.float64, rounded=False)
        v = ratio(got, mod, ref)
        rep["ratios"][key] = max(rep["ratios"].get(key, 0.0), v)
        _over(fails, "%s (layer %d)" % (key, l), v, ALLOWED[key], factor)
        lo, hi, single = mlp_interval(i, l, inp)
        inside = float(((got >= lo) & (got <= hi)).double().mean())
        rep["single"].append(single), rep["inside"].append(inside)
        if inside < 1.0:
            fails.append("layer %d: %.3g of the elements outside the derived interval" % (l, 1.0 - inside))
        if not torch.equal(bfr(got), got):
            fails.append("layer %d holds values that are no bf16" % l)
        if i["kind"] == "int" and not torch.equal(got, mod):
            fails.append("integer data: layer %d differs from the model" % l)
        if i["kind"] == "dead" and l < NL - 1 and float(got.abs().max()) != 0.0:
            fails.append("dead: hidden layer %d is not zero" % l)
    return fails, rep


def sum_bound_fraction(got, terms64_sum, mag, n):
    """largest |got - exact| as a fraction of n 2^-24 sum|term|; a sum of zeros must be zero"""
    err, bound = (got.double() - terms64_sum).abs(), n * U * mag
    if not bool((err[bound == 0] == 0).all()):
        return float("inf")
    return float((err / bound.clamp(min=1e-300))[bound > 0].max()) if bool((bound > 0).any()) else 0.0


def mlp_judge_bwd(i, hs, got, factor=1.0, mod_ref=None):
    """(fails, report) of dict(dx, dw, db) the kernel formed on the hidden outputs hs; mod_ref: (model, fp64) on hs if at hand"""
    fails, rep = [], dict(ratios={}, bound={}, agree=None)
    NL, N = i["NL"], i["N"]
    mod, ref = mod_ref or (mlp_backward(i, hs), mlp_backward(i, hs, torch.float64, rounded=False))

    def tight(key, name, g, m, r, floor):
        if not bool(torch.isfinite(g).all()):
            fails.append("%s not finite" % name)
            return
        v = ratio(g, m, r, floor) if g.dim() == 2 else vec_ratio(g, m, r)
        rep["ratios"][key] = max(rep["ratios"].get(key, 0.0), v)
        _over(fails, name, v, ALLOWED[key], factor)
        if i["kind"] == "int" and not torch.equal(g, m):
            fails.append("integer data: %s differs from the model" % name)

    if i["want_dx"]:
        tight("dx", "dx", got["dx"], mod["dx"], ref["dx"], None)
        rep["agree"] = float((got["dx"] == mod["dx"]).double().mean())
        if rep["agree"] < AGREE_MIN:
            fails.append("dx agrees with the model in %.3g of its elements only" % rep["agree"])
        if i["kind"] == "dead" and float(got["dx"].abs().max()) != 0.0:
            fails.append("dead: dx is not zero")
    for l in range(NL):
        tight("dw", "dw%d" % l, got["dw"][l], mod["dw"][l], ref["dw"][l], ulp_floor(ref["dw"][l]))
        if mod["db"][l] is not None:
            tight("db", "db%d" % l, got["db"][l], mod["db"][l], ref["db"][l], None)
        if i["kind"] == "dead" and l < NL - 1 and (float(got["dw"][l].abs().max()) != 0.0 or (got["db"][l] is not None and float(got["db"][l].abs().max()) != 0.0)):
            fails.append("dead: dw%d / db%d is not zero" % (l, l))
    # the top layer's sums against the terms the kernel adds
    dz, a = mod["dz_top"].double(), (i["x"] if NL == 1 else hs[NL - 2]).double()
    rep["bound"]["dw"] = sum_bound_fraction(got["dw"][NL - 1], dz.t() @ a, dz.abs().t() @ a.abs(), N)
    if mod["db"][NL - 1] is not None:
        rep["bound"]["db"] = sum_bound_fraction(got["db"][NL - 1], dz.sum(0), dz.abs().sum(0), N)
    for k, v in rep["bound"].items():
        if not v <= 1.0:
            fails.append("top-layer %s at %.3g of its derived bound" % (k, v))
    return fails, rep


@functools.lru_cache(maxsize=2)
def mlp_case(name):
    """dict(spec, inputs, routes, model_h, ref_h) of a named case; shared, read-only"""
    c = MLP_CASES[name]
    i = mlp_inputs(c, 2100 + sorted(MLP_CASES).index(name))
    return dict(spec=c, inputs=i, routes=mlp_case_routes(c), model_h=mlp_forward(i), ref_h=mlp_forward(i, torch.float64, rounded=False))


# ---------------------------------------------------------------------------------------------
# GRU gates: cases
# ---------------------------------------------------------------------------------------------
def _gru(dtype, N, C, **kw):
    c = dict(dtype=dtype, N=N, C=C, kind="randn", off={}, g_h=True, g_lp=True, out_lp=True)
    c.update(kw)
    return c


GRU_CASES = {}
for _dt in ("f32", "bf16"):
    _p = _dt[0]
    GRU_CASES.update({
        "v4_100_" + _p: _gru(_dt, 257, 100), "v4_4_" + _p: _gru(_dt, 1, 4), "s_7_" + _p: _gru(_dt, 5, 7), "s_30_" + _p: _gru(_dt, 130, 30),
        "trip2_v4_" + _p: _gru(_dt, 8193, 256),                      # 524352 lane groups > 2048 x 256
        "trip2_s_" + _p: _gru(_dt, 10487, 50),                       # 524350 elements, scalar
        "saturated_" + _p: _gru(_dt, 130, 64, kind="saturated"), "zero_state_" + _p: _gru(_dt, 65, 36, kind="zero_state"),
    })
GRU_CASES.update({
    "misaligned_gi_b": _gru("bf16", 257, 64, off={"gi": 1}),         # gi one element off: 2 bytes past an 8-byte boundary
    "misaligned_h_f": _gru("f32", 257, 64, off={"h": 1}),            # h one float off a 16-byte boundary
    "misaligned_glp_b": _gru("bf16", 257, 64, off={"g_lp": 1}),      # the backward alone goes scalar
    "g_h_only_b": _gru("bf16", 130, 64, g_lp=False), "g_lp_only_b": _gru("bf16", 130, 64, g_h=False),
    "no_out_lp_b": _gru("bf16", 130, 64, out_lp=False),
})
SAT_EVERY = 3                                                        # saturated: columns c % 3 == 0 carry |gi|, |gh| up to 12


def gru_case_routes(c, base=None):
    """(forward, backward) routes; every base on a 16-byte boundary but those moved by `off` elements.  base: the true addresses
    {name: address or None} of the GPU test."""
    s4 = 2 if c["dtype"] == "bf16" else 4
    size = dict(gi=s4, gh=s4, out_lp=s4, g_lp=s4, dgi=s4, dgh=s4, h=4, h_out=4, dh=4, g_h=4)
    a = {k: c["off"].get(k, 0) * size[k] for k in size} if base is None else dict(base)
    if not c["out_lp"]:
        a["out_lp"] = None
    if not c["g_lp"]:
        a["g_lp"] = None
    if not c["g_h"]:
        a["g_h"] = None
    fwd = gru_route(c["N"], c["C"], c["dtype"], dict(lp=(a["gi"], a["gh"], a["out_lp"]), f32=(a["h"], a["h_out"])))
    bwd = gru_route(c["N"], c["C"], c["dtype"], dict(lp=(a["gi"], a["gh"], a["g_lp"], a["dgi"], a["dgh"]), f32=(a["h"], a["dh"], a["g_h"])))
    return fwd, bwd


def gru_instances(c):
    """the hipLaunchKernelGGL instantiations of csrc/gru.hip a case runs"""
    fwd, bwd = gru_case_routes(c)
    return {("gru_gates_fwd_kernel", c["dtype"], fwd[0]), ("gru_gates_bwd_kernel", c["dtype"], bwd[0])}


def gru_inputs(c, seed):
    gen = torch.Generator().manual_seed(seed)
    rnd = lambda *s: torch.randn(*s, generator=gen)
    r = bfr if c["dtype"] == "bf16" else _ident
    N, C = c["N"], c["C"]
    gi, gh, h = rnd(N, 3 * C), rnd(N, 3 * C), rnd(N, C)
    if c["kind"] == "saturated":
        sat = (torch.arange(3 * C) % C) % SAT_EVERY == 0
        gi[:, sat] = (torch.rand(N, int(sat.sum()), generator=gen) * 24 - 12)
        gh[:, sat] = (torch.rand(N, int(sat.sum()), generator=gen) * 24 - 12)
    if c["kind"] == "zero_state":
        h = torch.zeros(N, C)
    return dict(N=N, C=C, bf16=c["dtype"] == "bf16", kind=c["kind"], gi=r(gi), gh=r(gh), h=h, g_h=rnd(N, C) if c["g_h"] else None,
                g_lp=r(rnd(N, C)) if c["g_lp"] else None, want_out_lp=c["out_lp"])


def _round_twice(t):
    """fp32 -> 19 significant bits (nearest even) -> bf16: a double rounding"""
    b = t.contiguous().view(torch.int32)
    mag, sign = b & 0x7fffffff, b & ~0x7fffffff
    mag = ((mag + 0xfff + ((mag >> 13) & 1)) >> 13) << 13
    return bfr((mag | sign).view(torch.float32))


def gru_compute(i, dt=torch.float32, rounded=True, mutation=None):
    """dict(h_out, out_lp, dgi, dgh, dh, floor) of one step in `dt`.  fp32 with rounded = True is the MODEL of csrc/gru.hip: the
    written-out step in fp32 on the stored gi / gh (torch's gate order r | z | n),
        r = 1 / (1 + exp(-(i_r + h_r))), z likewise, n = tanh(i_n + r h_n), h' = n + z (h - n), out_lp = h' rounded ONCE
        g = g_h + g_lp, dan = g (1 - z) (1 - n^2), daz = g (h - n) z (1 - z), dar = dan h_n r (1 - r)
        dgi = (dar | daz | dan), dgh = (dar | daz | dan r) rounded to the compute dtype, dh = g z in fp32
    (the device build contracts a + b c into an fma; the model need not).  `floor` [N]: the rms over a row of 2^-22 |g (1 - z)|,
    one fp32 ulp of 1 in n carried through 1 - n^2."""
    C = i["C"]
    r_ = bfr if (rounded and i["bf16"]) else _ident
    gi, gh, h = i["gi"].to(dt), i["gh"].to(dt), i["h"].to(dt)
    sig = lambda v: 1.0 / (1.0 + torch.exp(-v))
    o = (1, 0, 2) if mutation == "gate_order_zrn" else (0, 1, 2)
    ch = lambda t, k: t[:, o[k] * C:(o[k] + 1) * C]
    r, z = sig(ch(gi, 0) + ch(gh, 0)), sig(ch(gi, 1) + ch(gh, 1))
    hn = ch(gh, 2)
    n = torch.tanh((ch(gi, 2) + hn) * r) if mutation == "n_gate_r_outside" else torch.tanh(ch(gi, 2) + r * hn)
    h_out = n + z * (h - n)
    g = torch.zeros_like(h)
    if i["g_h"] is not None:
        g = g + i["g_h"].to(dt)
    if i["g_lp"] is not None and mutation != "g_lp_ignored":
        g = g + i["g_lp"].to(dt)
    dan = g * (1 - z) * (1 - n * n)
    daz = g * (h - n) * z * (1 - z)
    dar = dan * hn * r * (1 - r)
    parts = [None, None, None]
    parts[o[0]], parts[o[1]], parts[o[2]] = dar, daz, dan
    dgi = torch.cat(parts, 1)
    parts[o[2]] = dan if mutation == "dgh_n_without_r" else dan * r
    dgh = torch.cat(parts, 1)
    out = dict(h_out=h_out, dgi=r_(dgi), dgh=r_(dgh), dh=g if mutation == "dh_without_z" else g * z,
               floor=(2.0 ** -22 * (g * (1 - z)).double().abs()).pow(2).mean(dim=1).sqrt())
    if i["want_out_lp"]:
        out["out_lp"] = _round_twice(h_out.float()) if mutation == "out_lp_rounded_twice" else r_(h_out)
    if mutation == "tail_columns_dropped" and C % 4:
        k = C - C % 4
        for key in ("h_out", "dh", "out_lp"):
            if key in out:
                out[key] = out[key].clone()
                out[key][:, k:] = 0
        for key in ("dgi", "dgh"):
            out[key] = out[key].clone()
            for q in range(3):
                out[key][:, q * C + k:(q + 1) * C] = 0
    return out


def gru_judge(i, got, mod, ref, factor=1.0):
    """(fails, ratios) of dict(h_out, out_lp, dgi, dgh, dh) of the kernel"""
    fails, rat = [], {}
    for k in GRU_TENSORS:
        if not bool(torch.isfinite(got[k]).all()):
            fails.append("%s not finite" % k)
            continue
        floor = ref["floor"] if (i["kind"] == "saturated" and k in ("dgi", "dgh")) else None
        rat[k] = ratio(got[k], mod[k], ref[k], floor)
        _over(fails, k, rat[k], ALLOWED[k], factor)
    if i["want_out_lp"]:
        want = bfr(got["h_out"]) if i["bf16"] else got["h_out"]
        if not torch.equal(got["out_lp"], want):
            fails.append("out_lp is not h_out rounded once")
    return fails, rat


@functools.lru_cache(maxsize=2)
def gru_case(name):
    c = GRU_CASES[name]
    i = gru_inputs(c, 2300 + sorted(GRU_CASES).index(name))
    return dict(spec=c, inputs=i, routes=gru_case_routes(c), model=gru_compute(i), ref=gru_compute(i, torch.float64, rounded=False))


# ---------------------------------------------------------------------------------------------
# loss: cases
# ---------------------------------------------------------------------------------------------
def _loss(n, **kw):
    c = dict(n=n, n_total=n, data="randn", grad_off=1)
    c.update(kw)
    return c


LOSS_SHAPES = {"n%d" % n: _loss(n) for n in (1, 63, 64, 65, 1023, 1024, 1025, 8193)}
LOSS_SHAPES.update({"rows_%d" % t: _loss(200, n_total=200 + t) for t in (1, 1024, 3000)})
LOSS_SHAPES.update({"ties": _loss(1500, data="ties"), "int": _loss(5000, data="int"), "int_rows": _loss(5000, n_total=6100, data="int"),
                    "aligned": _loss(1025, grad_off=0)})            # (every other case: the gradient one float behind the loss, as ops.loss lays it out)
LOSS_CASES = {"%s_%s" % (s, k): dict(LOSS_SHAPES[s], shape=s, kind=q) for s in LOSS_SHAPES for q, k in enumerate(("l1", "mse"))}


def loss_inputs(c, seed):
    gen = torch.Generator().manual_seed(seed)
    n, nt = c["n"], c["n_total"]
    if c["data"] == "int":
        p, y = torch.randint(-8, 9, (nt,), generator=gen).float(), torch.randint(-8, 9, (n,), generator=gen).float()
    else:
        p, y = torch.randn(nt, generator=gen), torch.randn(n, generator=gen)
        if c["data"] == "ties":
            p[:n:3] = y[::3]
    return dict(n=n, n_total=nt, kind=c["kind"], p=p, y=y, data=c["data"])


def loss_compute(i, dt=torch.float32, mutation=None):
    """dict(loss, grad [n_total], terms): fp32 is the MODEL of loss_fwd_bwd_kernel: d = p - y, sum|d| or sum d^2 times fl(1 / n);
    gradient sign(d) fl(1 / n) (0 at a tie) or fl(2 d) fl(1 / n); exact zeros behind n.  fp64: the mean, the reference."""
    n, nt = i["n"], i["n_total"]
    p, y = i["p"][:n].to(dt), i["y"].to(dt)
    cnt = nt if mutation == "mean_over_n_total" else n
    inv = torch.tensor(1.0, dtype=dt) / torch.tensor(float(cnt), dtype=dt)
    d = p - y
    terms = d.abs() if i["kind"] == 0 else d * d
    keep = terms if mutation != "waves_dropped" else terms[(torch.arange(n) % 1024) < 64]
    grad = torch.zeros(nt, dtype=dt)
    if i["kind"] == 0:
        g = torch.sign(d) * inv
        if mutation == "tie_gradient_plus":
            g = torch.where(d == 0, inv.expand_as(g), g)
        grad[:n] = g
    else:
        grad[:n] = (2.0 * d) * inv
    if mutation == "tail_not_zeroed":
        grad[n:] = float("nan")
    return dict(loss=(keep.sum() * inv).reshape(1), grad=grad, terms=terms)


def loss_judge(i, got, mod, ref, factor=1.0):
    """(fails, report) of dict(loss [1], grad [n_total]) of the kernel"""
    fails, rep = [], {}
    n = i["n"]
    if not bool(torch.isfinite(got["loss"]).all()):
        return ["loss not finite"], rep
    rep["loss"] = vec_ratio(got["loss"], mod["loss"], ref["loss"])
    _over(fails, "loss", rep["loss"], ALLOWED["loss"], factor)
    t = mod["terms"].double()                                        # the fp32 terms the kernel adds
    err, bound = abs(float(got["loss"]) - float(t.sum()) / n), (n + 2) * U * float(t.abs().sum()) / n
    rep["bound"] = 0.0 if err == 0.0 else (err / bound if bound > 0 else float("inf"))
    if not rep["bound"] <= 1.0:
        fails.append("loss at %.3g of its derived bound" % rep["bound"])
    if not torch.equal(got["grad"][:n], mod["grad"][:n]):
        bad = (got["grad"][:n] != mod["grad"][:n]) | torch.isnan(got["grad"][:n])
        fails.append("gradient differs from fl(1/n) arithmetic in %d elements" % int(bad.sum()))
    if not bool((got["grad"][n:] == 0).all()):
        fails.append("the gradient behind n is not exactly zero")
    if i["data"] == "int" and not torch.equal(got["loss"].double(), mod["loss"].double()):
        fails.append("integer data: the loss differs from the model")
    return fails, rep


@functools.lru_cache(maxsize=4)
def loss_case(name):
    c = LOSS_CASES[name]
    i = loss_inputs(c, 2500 + sorted(LOSS_CASES).index(name))
    return dict(spec=c, inputs=i, model=loss_compute(i), ref=loss_compute(i, torch.float64))


# ---------------------------------------------------------------------------------------------
# mutations: kernel bugs in miniature.  name -> (family, applies(case spec), measure that owns it)
# ---------------------------------------------------------------------------------------------
_rand = lambda c: c["kind"] == "randn"
_NLm = lambda c: len(c["M"])
MUTATIONS = {
    # forward (mlp_forward, judged by mlp_judge_fwd)
    "drop_kstep": ("mlp_fwd", lambda c: _rand(c) and c["N"] >= 63 and (c["M"][0] if _NLm(c) > 1 else c["K0"]) >= 16),
    "skip_last_bias": ("mlp_fwd", lambda c: _rand(c) and (_NLm(c) - 1) not in c["nobias"]),
    "relu_last": ("mlp_fwd", lambda c: _rand(c) and c["N"] >= 63 and c["M"][-1] >= 2),      # (a 1-column y may hold no negative value)
    "hidden_fp32": ("mlp_fwd", lambda c: _rand(c) and _NLm(c) > 1 and c["N"] >= 63),
    "dirty_pad_columns": ("mlp_fwd", lambda c: _NLm(c) > 1 and min(c["M"][:-1]) < 64),
    # backward (mlp_backward on the model's hidden outputs, judged by mlp_judge_bwd)
    "mask_ge": ("mlp_bwd", lambda c: _rand(c) and _NLm(c) > 1 and c["N"] >= 63),
    "dz_not_rounded": ("mlp_bwd", lambda c: _rand(c) and _NLm(c) > 1 and c["dx"] and c["N"] >= 63 and c["K0"] >= 16),
    "gy_not_rounded": ("mlp_bwd", lambda c: c["f32io"]),
    "ragged_rows_missing": ("mlp_bwd", lambda c: c["kind"] in ("randn", "int") and c["N"] % 64 != 0 and c["N"] > 64),
    "trip2_rows_missing": ("mlp_bwd", lambda c: c["kind"] == "int" and c["N"] > 256 * 64),
    "nan_rows_included": ("mlp_bwd", lambda c: c["N"] % 64 != 0),
    "w_untransposed": ("mlp_bwd", lambda c: _rand(c) and c["N"] >= 63 and any(m == k for m, k in zip(c["M"], (c["K0"],) + c["M"][:-1])) and (c["dx"] or _NLm(c) > 1)),
    "db_wrong_layer": ("mlp_bwd", lambda c: _rand(c) and not c["nobias"] and any(a == b for a, b in zip(c["M"], c["M"][1:]))),
    # GRU
    "gate_order_zrn": ("gru", lambda c: c["kind"] != "zero_state"),
    "n_gate_r_outside": ("gru", lambda c: True),
    "dgh_n_without_r": ("gru", lambda c: True),
    "dh_without_z": ("gru", lambda c: True),
    "g_lp_ignored": ("gru", lambda c: c["g_lp"]),
    "out_lp_rounded_twice": ("gru", lambda c: c["dtype"] == "bf16" and c["out_lp"] and c["N"] * c["C"] >= 3000),
    "tail_columns_dropped": ("gru", lambda c: c["C"] % 4 != 0),
    # loss
    "mean_over_n_total": ("loss", lambda c: c["n_total"] > c["n"]),
    "tie_gradient_plus": ("loss", lambda c: c["data"] == "ties" and c["kind"] == 0),
    "tail_not_zeroed": ("loss", lambda c: c["n_total"] > c["n"]),
    "waves_dropped": ("loss", lambda c: c["n"] >= 65),
}


def mutated_fails(name, mutation):
    """the failures test_gpu_head_budget.py would report for the mutated model of a case, each ratio asked to stand 2 x ALLOWED"""
    fam = MUTATIONS[mutation][0]
    if fam == "mlp_fwd":
        k = mlp_case(name)
        return mlp_judge_fwd(k["inputs"], mlp_forward(k["inputs"], mutation=mutation), factor=2.0)[0]
    if fam == "mlp_bwd":
        k = mlp_case(name)
        return mlp_judge_bwd(k["inputs"], k["model_h"][:-1], mlp_backward(k["inputs"], k["model_h"][:-1], mutation=mutation), factor=2.0)[0]
    if fam == "gru":
        k = gru_case(name)
        return gru_judge(k["inputs"], gru_compute(k["inputs"], mutation=mutation), k["model"], k["ref"], factor=2.0)[0]
    k = loss_case(name)
    return loss_judge(k["inputs"], loss_compute(k["inputs"], mutation=mutation), k["model"], k["ref"], factor=2.0)[0]
