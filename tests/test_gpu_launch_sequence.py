"""The library entry points that one forward + backward of the CFConv / CGConv operators issues, by name and in order.

The host layer of matdeeplearn_amd/ops.py decides which kernels run and in which order; a change there that is meant to move
no launch is checked here.  For the duration of a case the cached library handle (_lib._lib) is replaced by a proxy whose
attributes are the real functions, wrapped to append their name to a list (size / capability queries included); the expected
lists below are literals, recorded on the commit in front of the one that introduced this file.  Every case runs under
ops.deterministic() on the random graph of the force tests (200 nodes, seed 17)."""
import pytest
import torch

import test_gpu_forces as tgf
from test_gpu_forces import dev

pytestmark = pytest.mark.gpu
N, G, SEED = 200, 50, 17


class _Recorder:
    def __init__(self, real, names):
        self._real, self._names = real, names

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def wrapped(*a):
            self._names.append(name)
            return fn(*a)
        return wrapped


def record(fn):
    """names of the library calls fn() makes"""
    from matdeeplearn_amd import _lib, ops
    real, names = _lib.lib(), []
    ops._tn_scratch(dev())                       # (allocated on first use per stream: keep its size query out of the lists)
    torch.cuda.synchronize()
    _lib._lib = _Recorder(real, names)
    try:
        with ops.deterministic():
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
