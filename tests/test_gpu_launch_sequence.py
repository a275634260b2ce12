"""The library entry points that one forward + backward of the CFConv / CGConv operators issues, by name and in order.

The host layer of matdeeplearn_amd/ops.py decides which kernels run and in which order; a change there that is meant to move
no launch is checked here.  For the duration of a case the cached library handle (_lib._lib) is replaced by a proxy whose
attributes are the real functions, wrapped to append their name to a list (size / capability queries included); the expected
lists below are literals, recorded on the commit in front of the one that introduced this file.  Every case runs under
ops.deterministic() on the random graph of the force tests (200 nodes, seed 17).

The dense layers (DENSE_CASES: the backward of ops.linear / linear_act / linear_gather_act / linear_relu_bn and the activation
hand-over of nn._seq) are recorded as (name, signature) in both modes, the default one and ops.deterministic(): the signature
lists every argument of the call — an int or float as its value, None or a null pointer as "-", any other pointer as "p" — so
strides, widths, row counts, activation / xout codes, flags and constants are pinned, addresses are not.  Their literals
(EXPECTED_DENSE) were recorded on the commit in front of the one that reduced the dense backward to one dispatch."""
import ctypes

import pytest
import torch

import test_gpu_forces as tgf
from test_gpu_forces import dev

pytestmark = pytest.mark.gpu
N, G, SEED = 200, 50, 17


def _signature(args):
    def one(a):
        if a is None or (isinstance(a, ctypes.c_void_p) and a.value is None):
            return "-"
        if isinstance(a, ctypes.c_void_p):
            return "p"
        if isinstance(a, (int, float)):
            return a
        return type(a).__name__
    return tuple(one(a) for a in args)


class _Recorder:
    def __init__(self, real, names, sig=False):
        self._real, self._names, self._sig = real, names, sig

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapped(*a):
            self._names.append((name, _signature(a)) if self._sig else name)
            return fn(*a)
        return wrapped


def record(fn, det=True, sig=False):
    """names of the library calls fn() makes (sig: (name, signature) pairs), in deterministic mode or the default one"""
    from matdeeplearn_amd import _lib, ops
    real, names = _lib.lib(), []
    ops._tn_scratch(dev())                       # (allocated on first use per stream: keep its size query out of the lists)
    torch.cuda.synchronize()
    _lib._lib = _Recorder(real, names, sig)
    try:
        with ops.deterministic(det):
            fn()
        torch.cuda.synchronize()
    finally:
        _lib._lib = real
    return names


def _graph(sort):
    from matdeeplearn_amd import ops
    ei = tgf.rand_graph(N, SEED, sort=sort).to(dev())
    return ei, ops.build_csr(ei, N, assume_sorted=sort)


def _rand(*shape, dtype=torch.float32, grad=False, scale=1.0, seed=0):
    t = (torch.randn(*shape, generator=torch.Generator().manual_seed(seed + sum(shape))) * scale).to(dev()).to(dtype)
    return t.requires_grad_(grad)


def _unit(*shape, dtype=torch.float32, grad=False, seed=0):
    t = torch.rand(*shape, generator=torch.Generator().manual_seed(seed + sum(shape))).to(dev()).to(dtype)
    return t.requires_grad_(grad)


def _lins(F):
    torch.manual_seed(F)
    return torch.nn.Linear(G, F).to(dev()), torch.nn.Linear(F, F).to(dev())


# --- SchNet's interaction block on the training path: two blocks, one BySourceAttrs -----------------------------------------
def _blocks(F):
    from matdeeplearn_amd import nn as mnn, ops
    C = 64
    _, csr = _graph(True)
    torch.manual_seed(F)
    blks = [mnn.InteractionBlock(C, G, F, 8.0).to(dev()) for _ in range(2)]
    x = _rand(N, C, dtype=torch.bfloat16, grad=True)
    ea, c, gout = _unit(csr.E, G, dtype=torch.bfloat16), _unit(csr.E), _rand(N, C, seed=1)

    def run():
        by_source = ops.BySourceAttrs()
        h = x
        for b in blks:
            h = b(h, None, None, ea, csr=csr, cut=c, by_source=by_source)
        (h.float() * gout).sum().backward()
    return run


# --- ops.cfconv: the node that is differentiable in the per-edge inputs ---------------------------------------------------------
def _cfconv(F, dtype, sort, dist):
    from matdeeplearn_amd import ops
    _, csr = _graph(sort)
    la, lb = _lins(F)
    h, gout = _rand(N, F, dtype=dtype, grad=True), _rand(N, F, seed=1)
    cut = _unit(csr.E, grad=True)
    if dist:
        dn = _unit(csr.E, grad=True, seed=2)
        offs = ops.rbf_offsets(0.0, 1.0, G, dev())
        rbf = ops.rbf_expand(dn.detach(), 0.0, 1.0, G, 0.2, out_dtype=dtype, offsets=offs)
        kw = {"dist": (dn, offs, ops.rbf_coeff(0.0, 1.0, 0.2))}
    else:
        rbf, kw = _unit(csr.E, G, dtype=dtype, grad=True), {}

    def run():
        out = ops.cfconv(rbf, cut, h, csr, la, lb, **kw)
        (out.float() * gout).sum().backward()
    return run


# --- ops.cgconv: the three backward tails, prepacked weights, the distance epilogue -------------------------------------------
def _cg_weights(C):
    k = 3.0 / (2 * C + G) ** 0.5
    return [_rand(C, 2 * C + G, grad=True, scale=k, seed=1), _rand(C, grad=True, scale=0.1, seed=2),
            _rand(C, 2 * C + G, grad=True, scale=k, seed=3), _rand(C, grad=True, scale=0.1, seed=4)]


def _cgconv(C, dtype, split=False, dist=False):
    from matdeeplearn_amd import ops
    ei, csr = _graph(True)
    w = _cg_weights(C)
    x, gout = _rand(N, C, dtype=dtype, grad=True), _rand(N, C, seed=1)
    if dist:
        dn = _unit(csr.E, grad=True, seed=2)
        offs = ops.rbf_offsets(0.0, 1.0, G, dev())
        ea = ops.rbf_expand(dn.detach(), 0.0, 1.0, G, 0.2, out_dtype=dtype, offsets=offs)
        kw = {"dist": (dn, offs, ops.rbf_coeff(0.0, 1.0, 0.2))}
    else:
        ea, kw = _unit(csr.E, G, dtype=dtype, grad=True), {}

    def run():
        out = ops.cgconv(x, ei, ea, *w, "mean", csr=csr, split=split, **kw)
        (out.float() * gout).sum().backward()
    return run


def _cgconv_prepacked():
    from matdeeplearn_amd import nn as mnn, ops
    C = 64
    ei, csr = _graph(True)
    torch.manual_seed(3)
    convs = [mnn.CGConv(C, G, aggr="mean", batch_norm=False).to(dev()) for _ in range(2)]
    x, gout = _rand(N, C, dtype=torch.bfloat16, grad=True), _rand(N, C, seed=1)
    ea = _unit(csr.E, G, dtype=torch.bfloat16, grad=True)

    def run():
        packs = ops.cgconv_prepack(convs, torch.bfloat16, dev())
        assert packs is not None
        h = x
        for cv, pk in zip(convs, packs):
            h = ops.cgconv(h, ei, ea, cv.lin_f.weight, cv.lin_f.bias, cv.lin_s.weight, cv.lin_s.bias, "mean", csr=csr, packed=pk)
        (h.float() * gout).sum().backward()
    return run


# --- the two stand-alone distance gradients, adding into a caller's buffer -----------------------------------------------------
def _cgconv_dist_grad():
    from matdeeplearn_amd import ops
    C = 64
    ei, csr = _graph(True)
    w = _cg_weights(C)
    x, gout, dn = _rand(N, C, dtype=torch.bfloat16), _rand(N, C, seed=1), _unit(csr.E, seed=2)
    buf = torch.zeros(csr.E, device=dev())
    return lambda: ops.cgconv_dist_grad(x, ei, dn, *w, gout, "mean", csr=csr, resolution=G, out=buf)


def _cfconv_dist_grad():
    from matdeeplearn_amd import ops
    F = 64
    ei, csr = _graph(True)
    la, lb = _lins(F)
    h, gout, dn, cut = _rand(N, F, dtype=torch.bfloat16), _rand(N, F, seed=1), _unit(csr.E, seed=2), _unit(csr.E)
    buf = torch.zeros(csr.E, device=dev())
    return lambda: ops.cfconv_dist_grad(h, ei, dn, cut, la.weight, la.bias, lb.weight, lb.bias, gout, csr=csr, resolution=G, out=buf,
                                        want_dcut=True)


CASES = {
    "block_bf16_F128_recompute": lambda: _blocks(128),
    "block_bf16_F64_stored": lambda: _blocks(64),
    "cfconv_dist_bf16_F64_unsorted": lambda: _cfconv(64, torch.bfloat16, False, True),
    "cfconv_dist_fp32_F150_unsorted": lambda: _cfconv(150, torch.float32, False, True),
    "cfconv_general_bf16_F64": lambda: _cfconv(64, torch.bfloat16, True, False),
    "cgconv_bf16_C64_node_hip": lambda: _cgconv(64, torch.bfloat16),
    "cgconv_bf16_C100_pad128": lambda: _cgconv(100, torch.bfloat16),
    "cgconv_fp32_C64_library": lambda: _cgconv(64, torch.float32, split=False),
    "cgconv_bf16_C64_prepacked": _cgconv_prepacked,
    "cgconv_bf16_C64_dist": lambda: _cgconv(64, torch.bfloat16, dist=True),
    "cgconv_dist_grad_out": _cgconv_dist_grad,
    "cfconv_dist_grad_out_dcut": _cfconv_dist_grad,
}

EXPECTED = {
    "block_bf16_F128_recompute": [
        "mdl_linear_act", "mdl_cfconv_supported", "mdl_cfconv_wpack_bytes", "mdl_cfconv_pack_weights", "mdl_cfconv_fwd",
        "mdl_linear_act", "mdl_linear_act", "mdl_linear_act", "mdl_cfconv_supported", "mdl_cfconv_wpack_bytes",
        "mdl_cfconv_pack_weights", "mdl_cfconv_fwd", "mdl_linear_act", "mdl_linear_act", "mdl_dense_bwd_ex", "mdl_dense_bwd_ex",
        "mdl_csr_rowptr", "mdl_gather_rows", "mdl_cfconv_fwd", "mdl_cfconv_bwd_w_scratch_bytes", "mdl_cfconv_bwd_w",
        "mdl_dense_bwd_ex", "mdl_dense_bwd_ex", "mdl_dense_bwd_ex", "mdl_cfconv_fwd", "mdl_cfconv_bwd_w_scratch_bytes",
        "mdl_cfconv_bwd_w", "mdl_dense_bwd_ex"
    ],
    "block_bf16_F64_stored": [
        "mdl_linear_act", "mdl_cfconv_supported", "mdl_cfconv_wpack_bytes", "mdl_cfconv_pack_weights", "mdl_cfconv_fwd",
        "mdl_linear_act", "mdl_linear_act", "mdl_linear_act", "mdl_cfconv_supported", "mdl_cfconv_wpack_bytes",
        "mdl_cfconv_pack_weights", "mdl_cfconv_fwd", "mdl_linear_act", "mdl_linear_act", "mdl_dense_bwd_ex", "mdl_dense_bwd_ex",
        "mdl_csr_rowptr", "mdl_gather_mul_reduce_dw", "mdl_dense_bwd_ex", "mdl_gemm_tn_ex", "mdl_dense_bwd_ex", "mdl_dense_bwd_ex",
        "mdl_dense_bwd_ex", "mdl_gather_mul_reduce_dw", "mdl_dense_bwd_ex", "mdl_gemm_tn_ex", "mdl_dense_bwd_ex"
    ],
    "cfconv_dist_bf16_F64_unsorted": [
        "mdl_cfconv_bwd_edge_supported", "mdl_cfconv_wpack_bytes", "mdl_cfconv_pack_weights", "mdl_cfconv_fwd", "mdl_csr_rowptr",
        "mdl_gather_rows", "mdl_cfconv_fwd", "mdl_cfconv_bwd_w_scratch_bytes", "mdl_cfconv_bwd_w", "mdl_cfconv_bwd_edge"
    ],
    "cfconv_dist_fp32_F150_unsorted": [
        "mdl_cfconv_bwd_edge_supported", "mdl_gather_mul_reduce", "mdl_csr_rowptr", "mdl_gather_mul_reduce", "mdl_edge_mul",
        "mdl_cfconv_bwd_edge"
    ],
    "cfconv_general_bf16_F64": [
        "mdl_cfconv_bwd_edge_supported", "mdl_cfconv_wpack_bytes", "mdl_cfconv_pack_weights", "mdl_cfconv_fwd", "mdl_csr_rowptr",
        "mdl_gather_rows", "mdl_cfconv_fwd", "mdl_cfconv_bwd_w_scratch_bytes", "mdl_cfconv_bwd_w", "mdl_cfconv_bwd_edge"
    ],
    "cgconv_bf16_C64_node_hip": [
        "mdl_cgconv_wpack_bytes", "mdl_cgconv_pack_weights_node", "mdl_cgconv_fwd_ex", "mdl_cgconv_bwd_edge",
        "mdl_cgconv_workspace_bytes", "mdl_cgconv_bwd_ex", "mdl_cgconv_bwd_node_ex", "mdl_cgconv_assemble_grads"
    ],
    "cgconv_bf16_C100_pad128": [
        "mdl_cgconv_wpack_bytes", "mdl_cgconv_pack_weights_node", "mdl_cgconv_fwd_ex", "mdl_cgconv_bwd_edge",
        "mdl_cgconv_workspace_bytes", "mdl_cgconv_bwd_ex", "mdl_gemm_tn_ex", "mdl_gemm_tn_ex", "mdl_gemm_tn_ex", "mdl_gemm_tn_ex",
        "mdl_cgconv_assemble_grads"
    ],
    "cgconv_fp32_C64_library": [
        "mdl_cgconv_wpack_bytes", "mdl_cgconv_pack_weights", "mdl_cgconv_fwd_ex", "mdl_cgconv_bwd_edge",
        "mdl_cgconv_workspace_bytes", "mdl_cgconv_bwd_ex"
    ],
    "cgconv_bf16_C64_prepacked": [
        "mdl_cgconv_wpack_bytes", "mdl_cgconv_pack_weights_multi", "mdl_cgconv_wpack_bytes", "mdl_cgconv_fwd_ex",
        "mdl_cgconv_wpack_bytes", "mdl_cgconv_fwd_ex", "mdl_cgconv_bwd_edge", "mdl_cgconv_workspace_bytes", "mdl_cgconv_bwd_ex",
        "mdl_cgconv_bwd_node_ex", "mdl_cgconv_assemble_grads", "mdl_cgconv_bwd_edge", "mdl_cgconv_workspace_bytes",
        "mdl_cgconv_bwd_ex", "mdl_cgconv_bwd_node_ex", "mdl_cgconv_assemble_grads"
    ],
    "cgconv_bf16_C64_dist": [
        "mdl_cgconv_wpack_bytes", "mdl_cgconv_pack_weights_node", "mdl_cgconv_fwd_ex", "mdl_cgconv_bwd_edge",
        "mdl_cgconv_workspace_bytes", "mdl_cgconv_bwd_ex", "mdl_cgconv_bwd_node_ex", "mdl_cgconv_assemble_grads"
    ],
    "cgconv_dist_grad_out": [
        "mdl_cgconv_wpack_bytes", "mdl_rbf_expand", "mdl_cgconv_wpack_bytes", "mdl_cgconv_pack_weights", "mdl_cgconv_bwd_edge"
    ],
    "cfconv_dist_grad_out_dcut": [
        "mdl_cfconv_bwd_edge_supported", "mdl_rbf_expand", "mdl_cfconv_wpack_bytes", "mdl_cfconv_pack_weights",
        "mdl_cfconv_bwd_edge"
    ],
}


@pytest.mark.parametrize("name", list(CASES))
def test_launch_sequence_is_what_it_was(name):
    got = record(CASES[name]())
    print(name, got)
    assert got == EXPECTED[name]


# --- the dense layers: one forward + backward on 130 rows (two 64-row tiles and two rows) -----------------------------------
ROWS, TABLE_ROWS = 130, 9
BF16 = torch.bfloat16


def _finish(out, gout, leaves):
    """the backward of sum(out * gout); returns the output and the gradient of every leaf (the bit-identity dumps read them)"""
    for t in leaves:
        t.grad = None
    (out.float() * gout).sum().backward()
    return [out.detach()] + [t.grad for t in leaves]


def _layer(M, K, x_grad=True):
    x = _rand(ROWS, K, dtype=BF16, grad=x_grad, seed=3)
    w, b = _rand(M, K, grad=True, scale=K ** -0.5, seed=4), _rand(M, grad=True, scale=0.1, seed=5)
    return x, w, b, _rand(ROWS, M, seed=6)


def _tables(M, count, grad=True):
    gen = torch.Generator().manual_seed(M + count)
    return [(_rand(TABLE_ROWS, M, grad=grad, scale=0.5, seed=7 + t),
             torch.randint(0, TABLE_ROWS, (ROWS,), generator=gen, dtype=torch.int32).to(dev())) for t in range(count)]


def _linear(M, K, x_grad=True):
    from matdeeplearn_amd import ops
    x, w, b, gout = _layer(M, K, x_grad)
    return lambda: _finish(ops.linear(x, w, b), gout, [x, w, b] if x_grad else [w, b])


def _linear_act(M, K, act):
    from matdeeplearn_amd import ops
    x, w, b, gout = _layer(M, K)
    return lambda: _finish(ops.linear_act(x, w, b, act), gout, [x, w, b])


def _gather(M, K, act, count, table_grad=True):
    from matdeeplearn_amd import ops
    x, w, b, gout = _layer(M, K)
    gath = _tables(M, count, table_grad)
    return lambda: _finish(ops.linear_gather_act(x, w, b, act, gath), gout, [x, w, b] + [t for t, _ in gath if table_grad])


def _relu_bn(name):
    import linear_budget
    from matdeeplearn_amd import ops
    _, rows, K, M, _, count, _, _ = linear_budget.LAYER_CASES[name]
    assert rows == ROWS
    x, w, b, gout = _layer(M, K)
    gath = _tables(M, count)
    gamma, beta = _unit(M, grad=True, seed=8), _rand(M, grad=True, scale=0.2, seed=9)
    gamma.data += 0.5
    rm, rv = torch.zeros(M, device=dev()), torch.ones(M, device=dev())

    def run():
        assert ops.linear_relu_bn_ok(x, w, True, gath or None)
        out = ops.linear_relu_bn(x, w, b, None, gamma, beta, rm, rv, 1e-5, 0.1, gath or None)
        return _finish(out, gout, [x, w, b, gamma, beta] + [t for t, _ in gath])
    return run


def _chain(widths, act):
    """nn._seq on Linear - act - Linear - act - ...: an activation behind every Linear but the last unless `widths` ends in None"""
    from matdeeplearn_amd import nn as mnn
    last_act = widths[-1] is None
    widths = [v for v in widths if v is not None]
    torch.manual_seed(sum(widths))
    mods = []
    for j in range(len(widths) - 1):
        mods.append(torch.nn.Linear(widths[j], widths[j + 1]))
        if j + 2 < len(widths) or last_act:
            mods.append(mnn.ShiftedSoftplus() if act == "ssp" else torch.nn.ReLU())
    seq = torch.nn.Sequential(*mods).to(dev())
    x, gout = _rand(ROWS, widths[0], dtype=BF16, grad=True, seed=3), _rand(ROWS, widths[-1], seed=6)
    return lambda: _finish(mnn._seq(seq, x), gout, [x] + list(seq.parameters()))


DENSE_CASES = {
    "linear_dense": lambda: _linear(64, 114),                          # _LinearTN on the one-pass backward
    "linear_no_dx": lambda: _linear(64, 114, x_grad=False),            # _LinearTN on TN GEMM + column sums
    "act_relu_odd_m": lambda: _linear_act(33, 64, "relu"),             # neither fused route: threshold_backward, odd-M padding
    "act_ssp_k160": lambda: _linear_act(32, 160, "ssp"),               # M < 34 and K > 158: the mdl_ssp_bwd fallback
    "gather_relu_dense": lambda: _gather(64, 66, "relu", 2),           # one-pass backward with gm, two segment sums
    "gather_relu_narrow": lambda: _gather(32, 160, "relu", 3),         # M < 34: mask + TN GEMM + three segment sums
    "gather_none": lambda: _gather(100, 66, None, 2),                  # no mask, g.contiguous() feeds the sums
    "gather_no_table_grad": lambda: _gather(64, 66, "relu", 2, table_grad=False),     # want_gm false
    "bn_0": lambda: _relu_bn("bn_0"),                                  # epilogue statistics, no table
    "bn_2": lambda: _relu_bn("bn_2"),                                  # epilogue statistics, two tables
    "bn_1": lambda: _relu_bn("bn_1"),                                  # separate statistics (one table)
    "chain_wide_ssp": lambda: _chain([64, 150, 150, 64], "ssp"),       # hand-over through xout of the one-pass backward
    # the hand-over on the route without the fused epilogue.  A chain that ENDS in a Linear never reaches mdl_linear_act_in with a
    # hand-over: its narrow layers either expect a pre-activation gradient (out_pre) or have no activation, so they take the
    # plain TN route.  The activation behind the last Linear(20, 64) puts that layer on the staged route (K = 20 < 34 keeps the
    # one-pass backward away): mdl_gemm_tn_ex with the activation, mdl_linear_act_in for dX, then the hand-over to Linear(64, 20),
    # which itself takes mdl_linear_act for dX and hands over to the first layer.
    "chain_narrow_relu": lambda: _chain([64, 64, 20, 64, None], "relu"),       # ... then threshold_backward(dx, x)
    "chain_narrow_ssp": lambda: _chain([64, 64, 20, 64, None], "ssp"),         # ... then the 1 - exp(-(x + ln2)) hand-over
}

EXPECTED_DENSE = {'linear_dense': {'default': [('mdl_dense_bwd_ex',
                               ('p', 64, 64, '-', 0, 0, 'p', 114, 114, 'p', 'p', 114, 0, '-', 'p', 'p', '-', 130, 1, '-'))],
                  'det': [('mdl_dense_bwd_ex',
                           ('p', 64, 64, '-', 0, 0, 'p', 114, 114, 'p', 'p', 114, 0, '-', 'p', 'p', '-', 130, 257, '-'))]},
 'linear_no_dx': {'default': [('mdl_gemm_tn_ex', ('p', 64, 64, '-', 0, 0, 'p', 114, 114, 'p', 'p', '-', 130, 1, '-'))],
                  'det': [('mdl_gemm_tn_ex', ('p', 64, 64, '-', 0, 0, 'p', 114, 114, 'p', 'p', '-', 130, 257, '-'))]},
 'act_relu_odd_m': {'default': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 33, 1, 1, '-')),
                                ('mdl_gemm_tn_ex', ('p', 34, 34, '-', 0, 0, 'p', 64, 64, 'p', 'p', '-', 130, 1, '-'))],
                    'det': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 33, 1, 1, '-')),
                            ('mdl_gemm_tn_ex', ('p', 34, 34, '-', 0, 0, 'p', 64, 64, 'p', 'p', '-', 130, 257, '-'))]},
 'act_ssp_k160': {'default': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 160, 32, 2, 1, '-')),
                              ('mdl_ssp_bwd', ('p', 'p', 'p', 4160, 1, '-')),
                              ('mdl_linear_act', ('p', 'p', '-', 'p', 130, 32, 160, 0, 1, '-')),
                              ('mdl_gemm_tn_ex', ('p', 32, 32, '-', 0, 0, 'p', 160, 160, 'p', '-', '-', 130, 1, '-'))],
                  'det': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 160, 32, 2, 1, '-')),
                          ('mdl_ssp_bwd', ('p', 'p', 'p', 4160, 1, '-')),
                          ('mdl_linear_act', ('p', 'p', '-', 'p', 130, 32, 160, 0, 1, '-')),
                          ('mdl_gemm_tn_ex', ('p', 32, 32, '-', 0, 0, 'p', 160, 160, 'p', '-', '-', 130, 257, '-'))]},
 'gather_relu_dense': {'default': [('mdl_linear_gather_act',
                                    ('p', 'p', 'p', 'p', 'p', 'p', 'p', '-', '-', 'p', 130, 66, 64, 1, 1, '-')),
                                   ('mdl_dense_bwd_ex',
                                    ('p', 64, 64, 'p', 64, 1, 'p', 66, 66, 'p', 'p', 66, 0, 'p', 'p', 'p', '-', 130, 1, '-')),
                                   ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                                   ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 64, 0, 1, '-')),
                                   ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                                   ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 64, 0, 1, '-'))],
                       'det': [('mdl_linear_gather_act',
                                ('p', 'p', 'p', 'p', 'p', 'p', 'p', '-', '-', 'p', 130, 66, 64, 1, 1, '-')),
                               ('mdl_dense_bwd_ex',
                                ('p', 64, 64, 'p', 64, 1, 'p', 66, 66, 'p', 'p', 66, 0, 'p', 'p', 'p', '-', 130, 257, '-')),
                               ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                               ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 64, 0, 1, '-')),
                               ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                               ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 64, 0, 1, '-'))]},
 'gather_relu_narrow': {'default': [('mdl_linear_gather_act',
                                     ('p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 130, 160, 32, 1, 1, '-')),
                                    ('mdl_linear_act', ('p', 'p', '-', 'p', 130, 32, 160, 0, 1, '-')),
                                    ('mdl_gemm_tn_ex', ('p', 32, 32, '-', 0, 0, 'p', 160, 160, 'p', '-', '-', 130, 1, '-')),
                                    ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                                    ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 32, 0, 1, '-')),
                                    ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                                    ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 32, 0, 1, '-')),
                                    ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                                    ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 32, 0, 1, '-'))],
                        'det': [('mdl_linear_gather_act',
                                 ('p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 130, 160, 32, 1, 1, '-')),
                                ('mdl_linear_act', ('p', 'p', '-', 'p', 130, 32, 160, 0, 1, '-')),
                                ('mdl_gemm_tn_ex', ('p', 32, 32, '-', 0, 0, 'p', 160, 160, 'p', '-', '-', 130, 257, '-')),
                                ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                                ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 32, 0, 1, '-')),
                                ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                                ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 32, 0, 1, '-')),
                                ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                                ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 32, 0, 1, '-'))]},
 'gather_none': {'default': [('mdl_linear_gather_act',
                              ('p', 'p', 'p', 'p', 'p', 'p', 'p', '-', '-', 'p', 130, 66, 100, 0, 1, '-')),
                             ('mdl_dense_bwd_ex',
                              ('p', 100, 100, '-', 0, 0, 'p', 66, 66, 'p', 'p', 66, 0, '-', 'p', 'p', '-', 130, 1, '-')),
                             ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                             ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 100, 0, 1, '-')),
                             ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                             ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 100, 0, 1, '-'))],
                 'det': [('mdl_linear_gather_act', ('p', 'p', 'p', 'p', 'p', 'p', 'p', '-', '-', 'p', 130, 66, 100, 0, 1, '-')),
                         ('mdl_dense_bwd_ex',
                          ('p', 100, 100, '-', 0, 0, 'p', 66, 66, 'p', 'p', 66, 0, '-', 'p', 'p', '-', 130, 257, '-')),
                         ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                         ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 100, 0, 1, '-')),
                         ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                         ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 100, 0, 1, '-'))]},
 'gather_no_table_grad': {'default': [('mdl_linear_gather_act',
                                       ('p', 'p', 'p', 'p', 'p', 'p', 'p', '-', '-', 'p', 130, 66, 64, 1, 1, '-')),
                                      ('mdl_dense_bwd_ex',
                                       ('p', 64, 64, 'p', 64, 1, 'p', 66, 66, 'p', 'p', 66, 0, '-', 'p', 'p', '-', 130, 1,
                                        '-'))],
                          'det': [('mdl_linear_gather_act',
                                   ('p', 'p', 'p', 'p', 'p', 'p', 'p', '-', '-', 'p', 130, 66, 64, 1, 1, '-')),
                                  ('mdl_dense_bwd_ex',
                                   ('p', 64, 64, 'p', 64, 1, 'p', 66, 66, 'p', 'p', 66, 0, '-', 'p', 'p', '-', 130, 257,
                                    '-'))]},
 'bn_0': {'default': [('mdl_bn_sums_rows', ()),
                      ('mdl_linear_act_stats',
                       ('p', 'p', 'p', '-', '-', '-', '-', '-', '-', 'p', 130, 64, 64, 1, 'p', '-', 1, '-')),
                      ('mdl_bn_apply_n', ('p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 130, 64, 1e-05, 0.1, '-', 2049, '-')),
                      ('mdl_bn_sums_rows', ()), ('mdl_bn_bwd_stats_n', ('p', 'p', 'p', 'p', 130, 64, '-', 1, '-')),
                      ('mdl_bn_bwd_apply_relu_n', ('p', 'p', 'p', 'p', 'p', 'p', 130, 64, '-', 1, '-')),
                      ('mdl_dense_bwd_ex',
                       ('p', 64, 64, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 1, '-'))],
          'det': [('mdl_bn_sums_rows', ()), ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 64, 1, 1, '-')),
                  ('mdl_bn_stats_n', ('p', 'p', 130, 64, '-', 257, '-')),
                  ('mdl_bn_apply_n', ('p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 130, 64, 1e-05, 0.1, '-', 1, '-')),
                  ('mdl_bn_sums_rows', ()), ('mdl_bn_bwd_stats_n', ('p', 'p', 'p', 'p', 130, 64, '-', 257, '-')),
                  ('mdl_bn_bwd_apply_relu_n', ('p', 'p', 'p', 'p', 'p', 'p', 130, 64, '-', 1, '-')),
                  ('mdl_dense_bwd_ex',
                   ('p', 64, 64, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 257, '-'))]},
 'bn_2': {'default': [('mdl_bn_sums_rows', ()),
                      ('mdl_linear_act_stats',
                       ('p', 'p', 'p', 'p', 'p', 'p', 'p', '-', '-', 'p', 130, 100, 36, 1, 'p', '-', 1, '-')),
                      ('mdl_bn_apply_n', ('p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 130, 36, 1e-05, 0.1, '-', 2049, '-')),
                      ('mdl_bn_sums_rows', ()), ('mdl_bn_bwd_stats_n', ('p', 'p', 'p', 'p', 130, 36, '-', 1, '-')),
                      ('mdl_bn_bwd_apply_relu_n', ('p', 'p', 'p', 'p', 'p', 'p', 130, 36, '-', 1, '-')),
                      ('mdl_dense_bwd_ex',
                       ('p', 36, 36, '-', 0, 0, 'p', 100, 100, 'p', 'p', 100, 0, '-', 'p', 'p', '-', 130, 1, '-')),
                      ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                      ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 36, 0, 1, '-')),
                      ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                      ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 36, 0, 1, '-'))],
          'det': [('mdl_bn_sums_rows', ()),
                  ('mdl_linear_gather_act', ('p', 'p', 'p', 'p', 'p', 'p', 'p', '-', '-', 'p', 130, 100, 36, 1, 1, '-')),
                  ('mdl_bn_stats_n', ('p', 'p', 130, 36, '-', 257, '-')),
                  ('mdl_bn_apply_n', ('p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 130, 36, 1e-05, 0.1, '-', 1, '-')),
                  ('mdl_bn_sums_rows', ()), ('mdl_bn_bwd_stats_n', ('p', 'p', 'p', 'p', 130, 36, '-', 257, '-')),
                  ('mdl_bn_bwd_apply_relu_n', ('p', 'p', 'p', 'p', 'p', 'p', 130, 36, '-', 1, '-')),
                  ('mdl_dense_bwd_ex',
                   ('p', 36, 36, '-', 0, 0, 'p', 100, 100, 'p', 'p', 100, 0, '-', 'p', 'p', '-', 130, 257, '-')),
                  ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                  ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 36, 0, 1, '-')),
                  ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                  ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 36, 0, 1, '-'))]},
 'bn_1': {'default': [('mdl_bn_sums_rows', ()),
                      ('mdl_linear_gather_act', ('p', 'p', 'p', 'p', 'p', '-', '-', '-', '-', 'p', 130, 64, 64, 1, 1, '-')),
                      ('mdl_bn_stats_n', ('p', 'p', 130, 64, '-', 1, '-')),
                      ('mdl_bn_apply_n', ('p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 130, 64, 1e-05, 0.1, '-', 1, '-')),
                      ('mdl_bn_sums_rows', ()), ('mdl_bn_bwd_stats_n', ('p', 'p', 'p', 'p', 130, 64, '-', 1, '-')),
                      ('mdl_bn_bwd_apply_relu_n', ('p', 'p', 'p', 'p', 'p', 'p', 130, 64, '-', 1, '-')),
                      ('mdl_dense_bwd_ex',
                       ('p', 64, 64, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 1, '-')),
                      ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                      ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 64, 0, 1, '-'))],
          'det': [('mdl_bn_sums_rows', ()),
                  ('mdl_linear_gather_act', ('p', 'p', 'p', 'p', 'p', '-', '-', '-', '-', 'p', 130, 64, 64, 1, 1, '-')),
                  ('mdl_bn_stats_n', ('p', 'p', 130, 64, '-', 257, '-')),
                  ('mdl_bn_apply_n', ('p', 'p', 'p', 'p', 'p', 'p', 'p', 'p', 130, 64, 1e-05, 0.1, '-', 1, '-')),
                  ('mdl_bn_sums_rows', ()), ('mdl_bn_bwd_stats_n', ('p', 'p', 'p', 'p', 130, 64, '-', 257, '-')),
                  ('mdl_bn_bwd_apply_relu_n', ('p', 'p', 'p', 'p', 'p', 'p', 130, 64, '-', 1, '-')),
                  ('mdl_dense_bwd_ex',
                   ('p', 64, 64, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 257, '-')),
                  ('mdl_csr_rowptr', ('p', 130, 9, 'p', '-')),
                  ('mdl_segment_reduce_fwd', ('p', 'p', 'p', 'p', '-', 9, 64, 0, 1, '-'))]},
 'chain_wide_ssp': {'default': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 150, 2, 1, '-')),
                                ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 150, 150, 2, 1, '-')),
                                ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 150, 64, 0, 1, '-')),
                                ('mdl_dense_bwd_ex',
                                 ('p', 64, 64, '-', 0, 0, 'p', 150, 150, 'p', 'p', 150, 2, '-', 'p', 'p', '-', 130, 1, '-')),
                                ('mdl_dense_bwd_ex',
                                 ('p', 150, 150, '-', 0, 0, 'p', 150, 150, 'p', 'p', 150, 2, '-', 'p', 'p', '-', 130, 1, '-')),
                                ('mdl_dense_bwd_ex',
                                 ('p', 150, 150, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 1, '-'))],
                    'det': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 150, 2, 1, '-')),
                            ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 150, 150, 2, 1, '-')),
                            ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 150, 64, 0, 1, '-')),
                            ('mdl_dense_bwd_ex',
                             ('p', 64, 64, '-', 0, 0, 'p', 150, 150, 'p', 'p', 150, 2, '-', 'p', 'p', '-', 130, 257, '-')),
                            ('mdl_dense_bwd_ex',
                             ('p', 150, 150, '-', 0, 0, 'p', 150, 150, 'p', 'p', 150, 2, '-', 'p', 'p', '-', 130, 257, '-')),
                            ('mdl_dense_bwd_ex',
                             ('p', 150, 150, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 257, '-'))]},
 'chain_narrow_relu': {'default': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 64, 1, 1, '-')),
                                   ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 20, 1, 1, '-')),
                                   ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 20, 64, 1, 1, '-')),
                                   ('mdl_gemm_tn_ex', ('p', 64, 64, 'p', 64, 1, 'p', 20, 20, 'p', 'p', '-', 130, 1, '-')),
                                   ('mdl_linear_act_in', ('p', 'p', 1, 'p', '-', 'p', 130, 64, 20, 0, 1, '-')),
                                   ('mdl_linear_act', ('p', 'p', '-', 'p', 130, 20, 64, 0, 1, '-')),
                                   ('mdl_gemm_tn_ex', ('p', 20, 20, '-', 0, 0, 'p', 64, 64, 'p', 'p', '-', 130, 1, '-')),
                                   ('mdl_dense_bwd_ex',
                                    ('p', 64, 64, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 1, '-'))],
                       'det': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 64, 1, 1, '-')),
                               ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 20, 1, 1, '-')),
                               ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 20, 64, 1, 1, '-')),
                               ('mdl_gemm_tn_ex', ('p', 64, 64, 'p', 64, 1, 'p', 20, 20, 'p', 'p', '-', 130, 257, '-')),
                               ('mdl_linear_act_in', ('p', 'p', 1, 'p', '-', 'p', 130, 64, 20, 0, 1, '-')),
                               ('mdl_linear_act', ('p', 'p', '-', 'p', 130, 20, 64, 0, 1, '-')),
                               ('mdl_gemm_tn_ex', ('p', 20, 20, '-', 0, 0, 'p', 64, 64, 'p', 'p', '-', 130, 257, '-')),
                               ('mdl_dense_bwd_ex',
                                ('p', 64, 64, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 257, '-'))]},
 'chain_narrow_ssp': {'default': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 64, 2, 1, '-')),
                                  ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 20, 2, 1, '-')),
                                  ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 20, 64, 2, 1, '-')),
                                  ('mdl_gemm_tn_ex', ('p', 64, 64, 'p', 64, 2, 'p', 20, 20, 'p', 'p', '-', 130, 1, '-')),
                                  ('mdl_linear_act_in', ('p', 'p', 2, 'p', '-', 'p', 130, 64, 20, 0, 1, '-')),
                                  ('mdl_linear_act', ('p', 'p', '-', 'p', 130, 20, 64, 0, 1, '-')),
                                  ('mdl_gemm_tn_ex', ('p', 20, 20, '-', 0, 0, 'p', 64, 64, 'p', 'p', '-', 130, 1, '-')),
                                  ('mdl_dense_bwd_ex',
                                   ('p', 64, 64, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 1, '-'))],
                      'det': [('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 64, 2, 1, '-')),
                              ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 64, 20, 2, 1, '-')),
                              ('mdl_linear_act', ('p', 'p', 'p', 'p', 130, 20, 64, 2, 1, '-')),
                              ('mdl_gemm_tn_ex', ('p', 64, 64, 'p', 64, 2, 'p', 20, 20, 'p', 'p', '-', 130, 257, '-')),
                              ('mdl_linear_act_in', ('p', 'p', 2, 'p', '-', 'p', 130, 64, 20, 0, 1, '-')),
                              ('mdl_linear_act', ('p', 'p', '-', 'p', 130, 20, 64, 0, 1, '-')),
                              ('mdl_gemm_tn_ex', ('p', 20, 20, '-', 0, 0, 'p', 64, 64, 'p', 'p', '-', 130, 257, '-')),
                              ('mdl_dense_bwd_ex',
                               ('p', 64, 64, '-', 0, 0, 'p', 64, 64, 'p', 'p', 64, 0, '-', 'p', 'p', '-', 130, 257, '-'))]}}


@pytest.mark.parametrize("det", [False, True], ids=["default", "det"])
@pytest.mark.parametrize("name", list(DENSE_CASES))
def test_dense_launch_sequence_is_what_it_was(name, det):
    got = record(DENSE_CASES[name](), det=det, sig=True)
    print(name, "det" if det else "default", got)
    assert got == EXPECTED_DENSE[name]["det" if det else "default"]
