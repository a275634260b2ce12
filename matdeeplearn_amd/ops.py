"""Host-side operators over libmdl_hip.so: CSR graph index, RBF expansion, scatter / pooling, CGConv.

These mirror the third-party operator API the reference calls (level b2):
  scatter / scatter_mean / scatter_add  <- torch_scatter      (matdeeplearn/models/megnet.py:13,86,130-132,342-348)
  global_{mean,add,max}_pool            <- torch_geometric.nn (matdeeplearn/models/cgcnn.py:154)
  cgconv                                <- torch_geometric.nn.CGConv.forward (matdeeplearn/models/cgcnn.py:136-145)
  rbf_expand                            <- GaussianSmearing.forward (matdeeplearn/process/process.py:588-590)
Same argument meaning, differentiable through torch.autograd.Function, errors raised as Python
exceptions.  Every op runs a hand-written HIP kernel; there is no eager/CPU fallback.
"""
import collections
import os
import weakref

import numpy as np
import torch

from . import _lib
from ._lib import MdlError, check, dtype_code, lib, ptr, require_hip, stream

_ACT_CODE = {"relu": 1, "ssp": 2}        # activation codes of the dense kernels (0 = none)
_LN2 = 0.6931471805599453                # the shift of the shifted softplus


def _f32c(t):
    """t as a detached, contiguous fp32 tensor (None stays None): how the packing kernels read weights and biases"""
    return None if t is None else t.detach().float().contiguous()


def _stream_key(device):
    """key of the per-device, per-stream buffer tables"""
    return (device.index, torch.cuda.current_stream(device).cuda_stream)


# ------------------------------------------------------------------------------------------------
# CSR-by-target graph index
# ------------------------------------------------------------------------------------------------
class EdgeCSR:
    """Edges sorted by target.  rowptr [N+1], src/tgt [E] int32, eperm [E] int32 or None when the
    caller's per-edge tensors are already in CSR order (the product loader guarantees that)."""

    __slots__ = ("rowptr", "src", "tgt", "eperm", "N", "E", "_row", "_col", "_t", "_attr", "_tb", "_bal", "partial", "__weakref__")

    def __init__(self, rowptr, src, tgt, eperm, N, E, row=None, col=None):
        self.rowptr, self.src, self.tgt, self.eperm, self.N, self.E = rowptr, src, tgt, eperm, int(N), int(E)
        self._attr = None
        self._bal = None
        self._row, self._col, self._t, self._tb = row, col, None, None
        self.partial = False      # padded static batch: the arrays hold more rows than the rowptr ranges cover

    def set_transposed(self, t):
        """(rowptr_s, col_s, eid_s, src_sorted) supplied by the loader (static buffers of the HIP-graph path)."""
        self._t = tuple(t)

    def set_transposed_builder(self, fn):
        """fn() -> (rowptr_s, col_s, eid_s, src_sorted): the loader's sort-free construction, run on first use."""
        self._tb = fn

    def balance(self):
        """[N + 1] int32 cost prefix for the work distribution of the edge-per-lane CGConv backward (mdl_cgconv_balance + one
        cumsum): topology only, so it is built once per batch and serves every layer."""
        if self._bal is None:
            cost = torch.empty(self.N + 1, dtype=torch.int32, device=self.rowptr.device)
            check(lib().mdl_cgconv_balance(ptr(self.rowptr), ptr(self.src), self.N, ptr(cost), stream()), "mdl_cgconv_balance")
            self._bal = torch.cumsum(cost, 0, dtype=torch.int32)
        return self._bal

    def refresh_balance(self):
        """A CSR over static buffers (HIP-graph path) is rewritten in place with every batch: its prefix is rebuilt into the
        SAME tensor by the batch assembly, inside the captured graph."""
        if not (_BALANCE and self.E >= 400000 and self.eperm is None):
            return
        if self._bal is None:
            self._bal = torch.zeros(self.N + 1, dtype=torch.int32, device=self.rowptr.device)
        cost = torch.empty(self.N + 1, dtype=torch.int32, device=self.rowptr.device)
        check(lib().mdl_cgconv_balance(ptr(self.rowptr), ptr(self.src), self.N, ptr(cost), stream()), "mdl_cgconv_balance")
        torch.cumsum(cost, 0, dtype=torch.int32, out=self._bal)

    def seg_tgt(self):
        """segment index of `col` (target per edge): what scatter(..., index=edge_index[1]) needs, without a sort"""
        if self.eperm is not None:
            return None
        return make_seg_index(self.rowptr, self.tgt, partial=self.partial)

    def seg_src(self):
        """segment index of `row` (source per edge) from the by-source CSR"""
        if self.eperm is not None:
            return None
        rowptr_s, _, eid_s, src_sorted = self.transposed()
        si = make_seg_index(rowptr_s, src_sorted, partial=self.partial)
        si.perm = eid_s
        return si

    def sorted_attr(self, edge_attr):
        """edge_attr rows in CSR (target-sorted) order.  The static CGConv kernels stream the edge features
        sequentially, so an unsorted edge list is permuted ONCE per (edge_attr, CSR) here (cached; edge_attr
        is constant across the layers of a model) instead of being gathered through eperm in every launch."""
        if self.eperm is None:
            return edge_attr
        k = (edge_attr.data_ptr(), edge_attr._version, edge_attr.dtype, tuple(edge_attr.shape))
        if self._attr is None or self._attr[0] != k:
            self._attr = (k, edge_attr.index_select(0, self.eperm.long()).contiguous(), edge_attr)
        return self._attr[1]

    @property
    def row(self):
        """source of every edge in the CALLER's edge order (int32)"""
        if self._row is None:
            self._row = _unsort_edges(self.src, self)
        return self._row

    @property
    def col(self):
        """target of every edge in the caller's edge order (int32)"""
        if self._col is None:
            self._col = _unsort_edges(self.tgt, self)
        return self._col

    def transposed(self):
        """CSR by SOURCE: (rowptr_s [N+1], col_s = target per slot, eid_s = caller's edge id per slot)."""
        if self._t is None and self._tb is not None:
            self._t = tuple(self._tb())
        if self._t is None:
            perm = torch.argsort(self.src, stable=True)
            src_sorted = self.src.index_select(0, perm)
            col_s = self.tgt.index_select(0, perm)
            eid_s = (perm if self.eperm is None else self.eperm.long().index_select(0, perm)).to(torch.int32)
            self._t = (csr_rowptr(src_sorted.contiguous(), self.N), col_s.contiguous(), eid_s.contiguous(),
                       src_sorted.contiguous())
        return self._t


def csr_rowptr(sorted_index_i32, num_segments):
    require_hip(sorted_index_i32)
    rowptr = torch.empty(num_segments + 1, dtype=torch.int32, device=sorted_index_i32.device)
    check(lib().mdl_csr_rowptr(ptr(sorted_index_i32), sorted_index_i32.numel(), num_segments, ptr(rowptr), stream()),
          "mdl_csr_rowptr")
    return rowptr


def build_csr(edge_index, num_nodes, assume_sorted=False):
    """edge_index: [2, E] int64/int32 (row 0 = source j, row 1 = target i).  No host sync."""
    require_hip(edge_index)
    row, col = edge_index[0], edge_index[1]
    if assume_sorted:
        tgt = col.to(torch.int32).contiguous()
        src = row.to(torch.int32).contiguous()
        eperm = None
    else:
        perm = torch.argsort(col, stable=True)
        tgt = col.index_select(0, perm).to(torch.int32)
        src = row.index_select(0, perm).to(torch.int32)
        eperm = perm.to(torch.int32)
    return EdgeCSR(csr_rowptr(tgt, num_nodes), src, tgt, eperm, num_nodes, col.numel(),
                   row=None if assume_sorted else row.to(torch.int32).contiguous(),
                   col=None if assume_sorted else col.to(torch.int32).contiguous())


_CSR_CACHE = collections.OrderedDict()
_CSR_CACHE_MAX = 64                      # entries
_CSR_CACHE_MAX_BYTES = 256 << 20         # and bytes pinned (an entry keeps ~40 B/edge of index tensors alive)
_csr_cache_bytes = 0


def _key(edge_index, n):
    return (edge_index.data_ptr(), edge_index._version, tuple(edge_index.shape), int(n), edge_index.device.index)


def _csr_entry_bytes(edge_index, csr):
    return edge_index.numel() * edge_index.element_size() + 4 * (3 * csr.E + csr.N + 1) + (4 * csr.E if csr.eperm is not None else 0)


def register_csr(edge_index, csr):
    """Attach a pre-built CSR to an edge_index tensor (used by the product loader).  The cache is bounded by entries AND
    by the device bytes it pins; the newest entry always stays."""
    global _csr_cache_bytes
    k = _key(edge_index, csr.N)
    old = _CSR_CACHE.pop(k, None)
    if old is not None:
        _csr_cache_bytes -= old[2]
    nb = _csr_entry_bytes(edge_index, csr)
    _CSR_CACHE[k] = (csr, edge_index, nb)  # keep the tensor alive so data_ptr cannot be recycled
    _csr_cache_bytes += nb
    while len(_CSR_CACHE) > 1 and (len(_CSR_CACHE) > _CSR_CACHE_MAX or _csr_cache_bytes > _CSR_CACHE_MAX_BYTES):
        _csr_cache_bytes -= _CSR_CACHE.popitem(last=False)[1][2]


def csr_for(edge_index, num_nodes):
    """CSR of a PyG-style edge_index; built on first use (device sort) and cached per tensor."""
    if NO_INDEX_CACHE:
        return build_csr(edge_index, num_nodes)
    k = _key(edge_index, num_nodes)
    hit = _CSR_CACHE.get(k)
    if hit is not None:
        _CSR_CACHE.move_to_end(k)
        return hit[0]
    csr = build_csr(edge_index, num_nodes)
    register_csr(edge_index, csr)
    return csr


# ------------------------------------------------------------------------------------------------
# K1 — Gaussian RBF expansion
# ------------------------------------------------------------------------------------------------
def rbf_offsets(start=0.0, stop=1.0, resolution=50, device=None):
    """process.py:583 — the fp32 torch.linspace centre buffer (computed on the host so the grid is
    bit-identical to the reference's, then uploaded)."""
    return torch.linspace(start, stop, resolution).to(device)


def rbf_coeff(start=0.0, stop=1.0, width=0.2):
    return -0.5 / ((stop - start) * width) ** 2  # process.py:585


class _RbfExpand(torch.autograd.Function):
    """rbf_expand for distances that require a gradient: the same forward launch, mdl_rbf_expand_bwd behind it."""

    @staticmethod
    def forward(ctx, dist, offsets, coeff, out_dtype):
        E, G = dist.numel(), offsets.numel()
        out = torch.empty((E, G), dtype=out_dtype, device=dist.device)
        check(lib().mdl_rbf_expand(ptr(dist), ptr(offsets), coeff, ptr(out), E, G, G, dtype_code(out), stream()), "mdl_rbf_expand")
        ctx.save_for_backward(dist, offsets)
        ctx.coeff = coeff
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        dist, offsets = ctx.saved_tensors
        g = g.contiguous()
        E, G = g.shape
        dd = torch.empty(E, dtype=torch.float32, device=g.device)
        check(lib().mdl_rbf_expand_bwd(ptr(g), G, dtype_code(g), ptr(dist), ptr(offsets), ctx.coeff, ptr(dd), E, G, stream()),
              "mdl_rbf_expand_bwd")
        return dd, None, None, None


def rbf_expand(dist, start=0.0, stop=1.0, resolution=50, width=0.2, out_dtype=torch.float32, offsets=None,
               out=None):
    """GaussianSmearing(start, stop, resolution, width)(dist): [E] fp32 -> [E, resolution].
    Differentiable w.r.t. dist (first order: the backward recomputes the Gaussians from dist and raises on a second
    differentiation); distances that do not require a gradient run the one launch they always did."""
    require_hip(dist)
    if dist.dtype != torch.float32:
        raise MdlError("rbf_expand: distances must be float32")
    dist = dist.contiguous()
    if offsets is None:
        offsets = rbf_offsets(start, stop, resolution, dist.device)
    if dist.requires_grad and torch.is_grad_enabled():
        if out is not None:
            raise MdlError("rbf_expand: out= cannot be combined with distances that require a gradient")
        return _RbfExpand.apply(dist, offsets.contiguous(), float(rbf_coeff(start, stop, width)), out_dtype)
    E, G = dist.numel(), offsets.numel()
    if out is None:
        out = torch.empty((E, G), dtype=out_dtype, device=dist.device)
    check(lib().mdl_rbf_expand(ptr(dist), ptr(offsets), float(rbf_coeff(start, stop, width)), ptr(out), E, G,
                               out.stride(0) if E else G, dtype_code(out), stream()), "mdl_rbf_expand")
    return out


# ------------------------------------------------------------------------------------------------
# K5 — scatter / pooling over a sorted (or sortable) index
# ------------------------------------------------------------------------------------------------
class _SegIndex:
    __slots__ = ("rowptr", "seg", "perm", "N", "E", "partial")


_SEG_CACHE = collections.OrderedDict()
# index tensors whose segment index the loader already knows (edge_index rows of a product batch: no sort, and the only
# correct index for the static buffers of the HIP-graph path, whose unused tail must stay outside every segment)
_SEG_KNOWN = collections.OrderedDict()


def register_seg_index(index, si, owner=None):
    """`scatter(src, index, ...)` calls with this very memory (same address and length) use `si` — a segment index or a
    callable that builds it on first use — for as long as `owner` (the tensor that owns the storage; default `index`)
    is alive.  Only a weak reference is kept: when the owner dies its address may be recycled and the entry is dropped."""
    import weakref
    _SEG_KNOWN[(index.data_ptr(), index.numel(), index.device.index)] = [si, weakref.ref(index if owner is None else owner)]
    while len(_SEG_KNOWN) > 64:
        _SEG_KNOWN.popitem(last=False)


def _known_seg_index(index, dim_size):
    key = (index.data_ptr(), index.numel(), index.device.index)
    ent = _SEG_KNOWN.get(key)
    if ent is None:
        return None
    if ent[1]() is None:
        del _SEG_KNOWN[key]
        return None
    si = ent[0]() if callable(ent[0]) else ent[0]     # (a callable is resolved per use: the registry must not pin a batch)
    return si if (si is not None and si.N == int(dim_size)) else None


# Static buffers (HIP-graph path) are rewritten in place by kernels the version counter does not see: with NO_INDEX_CACHE
# every index structure is rebuilt (and the building kernels become part of the captured graph).
NO_INDEX_CACHE = False


def _seg_index(index, dim_size, assume_sorted):
    known = _known_seg_index(index, dim_size)
    if known is not None:
        return known
    if NO_INDEX_CACHE:
        return _seg_index_build(index, dim_size, assume_sorted)
    key = (index.data_ptr(), index._version, index.numel(), int(dim_size), bool(assume_sorted), index.device.index)
    hit = _SEG_CACHE.get(key)
    if hit is not None:
        return hit[0]
    si = _seg_index_build(index, dim_size, assume_sorted)
    _SEG_CACHE[key] = (si, index)
    while len(_SEG_CACHE) > 64:
        _SEG_CACHE.popitem(last=False)
    return si


def _seg_index_build(index, dim_size, assume_sorted):
    si = _SegIndex()
    si.N, si.E, si.partial = int(dim_size), index.numel(), False
    if assume_sorted:
        si.seg, si.perm = index.to(torch.int32).contiguous(), None
    else:
        perm = torch.argsort(index, stable=True)
        si.seg, si.perm = index.index_select(0, perm).to(torch.int32), perm.to(torch.int32)
    si.rowptr = csr_rowptr(si.seg, si.N)
    return si


class _SegmentReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, si, reduce):
        require_hip(src)
        src = src.contiguous()
        C = src.numel() // max(src.shape[0], 1) if src.dim() > 1 else 1
        out = torch.empty((si.N,) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
        argmax = torch.empty((si.N, C), dtype=torch.int32, device=src.device) if reduce == _lib.MDL_MAX else None
        check(lib().mdl_segment_reduce_fwd(ptr(src), ptr(si.rowptr), ptr(si.perm), ptr(out), ptr(argmax), si.N, C,
                                           reduce, dtype_code(src), stream()), "mdl_segment_reduce_fwd")
        ctx.si, ctx.reduce, ctx.C, ctx.shape = si, reduce, C, tuple(src.shape)
        ctx.save_for_backward(argmax) if argmax is not None else ctx.save_for_backward()
        return out

    @staticmethod
    def backward(ctx, g):
        si, C = ctx.si, ctx.C
        g = g.contiguous()
        argmax = ctx.saved_tensors[0] if ctx.reduce == _lib.MDL_MAX else None
        # rows outside every segment (the unused tail of a padded static batch) must get exact zeros: they feed dense
        # per-row kernels (weight-gradient GEMMs) that run over all rows.  The sum / mean kernels write EVERY row from g[seg[row]],
        # and a padded row's segment id is the dummy graph / the first padding node, whose gradient row is exactly zero by the
        # static batch's invariant — so only the max form (which writes the argmax rows alone) needs the fill launch
        alloc = torch.zeros if ctx.reduce == _lib.MDL_MAX else torch.empty
        gs = alloc(ctx.shape, dtype=g.dtype, device=g.device)
        check(lib().mdl_segment_reduce_bwd(ptr(g), ptr(si.rowptr), ptr(si.seg), ptr(si.perm), ptr(argmax), ptr(gs),
                                           si.N, si.E, C, ctx.reduce, dtype_code(g), stream()),
              "mdl_segment_reduce_bwd")
        return gs, None, None


class _ResidualSegmentReduce(torch.autograd.Function):
    """(src + res, reduce(src by segment)) as one autograd node: `src` feeds a residual sum AND a segmented reduction (the edge
    state of a MEGNet block: e' + e and scatter_mean(e', row), megnet.py:86 with :321-336), so its gradient is the sum of two
    [E, C] tensors — formed here inside the reduction's backward (mdl_segment_reduce_bwd_add) instead of by autograd's
    separate accumulation pass."""

    @staticmethod
    def forward(ctx, src, res, si, reduce):
        C = src.shape[1]
        out = torch.empty((si.N, C), dtype=src.dtype, device=src.device)
        check(lib().mdl_segment_reduce_fwd(ptr(src), ptr(si.rowptr), ptr(si.perm), ptr(out), None, si.N, C, reduce,
                                           dtype_code(src), stream()), "mdl_segment_reduce_fwd")
        ctx.si, ctx.reduce = si, reduce
        return src + res, out

    @staticmethod
    def backward(ctx, g_sum, g_red):
        si = ctx.si
        g_sum, g_red = g_sum.contiguous(), g_red.contiguous()
        gs = torch.empty_like(g_sum)
        check(lib().mdl_segment_reduce_bwd_add(ptr(g_red), ptr(si.rowptr), ptr(si.seg), ptr(si.perm), ptr(g_sum), ptr(gs),
                                               si.N, si.E, g_sum.shape[1], ctx.reduce, dtype_code(g_sum), stream()),
              "mdl_segment_reduce_bwd_add")
        return gs, g_sum, None, None


def residual_scatter(src, res, index, dim_size, reduce="mean", assume_sorted=False):
    """(src + res, scatter(src, index, 0, dim_size, reduce)) — one node when the shapes allow (2-D contiguous rows of a
    multiple of 4 elements, sum / mean, an index whose segments cover every row), the two separate ops otherwise."""
    if (reduce in ("sum", "mean") and src.dim() == 2 and src.is_cuda and src.is_contiguous() and res.is_contiguous()
            and res.shape == src.shape and res.dtype == src.dtype and src.shape[1] % 4 == 0 and src.data_ptr() % 16 == 0
            and src.shape[0] > 0 and torch.is_grad_enabled() and src.requires_grad):
        require_hip(src, index)
        si = _seg_index(index, dim_size, assume_sorted)
        if not si.partial and si.E == src.shape[0]:
            return _ResidualSegmentReduce.apply(src, res, si, _lib.REDUCE[reduce])
    return src + res, scatter(src, index, 0, dim_size, reduce, assume_sorted)


def scatter(src, index, dim=0, dim_size=None, reduce="sum", assume_sorted=False, seg_index=None):
    """torch_scatter.scatter(src, index, dim=0, dim_size, reduce) semantics.  When
    dim_size is None it is index.max()+1, which costs a host sync — pass dim_size on hot paths.
    `seg_index`: a prebuilt segment index (make_seg_index) for `index`, e.g. the loader's node -> graph map."""
    if dim != 0:
        raise MdlError("scatter: only dim=0 is on the hot path")
    require_hip(src, index)
    if reduce not in _lib.REDUCE:
        raise MdlError("scatter: unsupported reduce %r" % (reduce,))
    if seg_index is None:
        if dim_size is None:
            dim_size = int(index.max()) + 1 if index.numel() else 0
        seg_index = _seg_index(index, dim_size, assume_sorted)
    return _SegmentReduce.apply(src, seg_index, _lib.REDUCE[reduce])


def make_seg_index(rowptr_i32, seg_i32, partial=False):
    """Segment index over a SORTED segment id vector from its row pointers (rowptr [S+1] int32, seg [E] int32): what the
    loaders know anyway (graph -> first node), so pooling needs neither a sort nor a search.  partial: the rowptr ranges
    do not cover all E rows (padded static batch)."""
    si = _SegIndex()
    si.N, si.E, si.partial = rowptr_i32.numel() - 1, seg_i32.numel(), bool(partial)
    si.rowptr, si.seg, si.perm = rowptr_i32, seg_i32, None
    return si


def scatter_mean(src, index, dim=0, dim_size=None, assume_sorted=False):
    return scatter(src, index, dim, dim_size, "mean", assume_sorted)


def scatter_add(src, index, dim=0, dim_size=None, assume_sorted=False):
    return scatter(src, index, dim, dim_size, "sum", assume_sorted)


def global_mean_pool(x, batch, size=None, seg_index=None):
    """`batch` is non-decreasing by construction (PyG collate / the product loader)."""
    return scatter(x, batch, 0, size, "mean", assume_sorted=True, seg_index=seg_index)


def global_add_pool(x, batch, size=None, seg_index=None):
    return scatter(x, batch, 0, size, "sum", assume_sorted=True, seg_index=seg_index)


def global_max_pool(x, batch, size=None, seg_index=None):
    return scatter(x, batch, 0, size, "max", assume_sorted=True, seg_index=seg_index)


POOLS = {"global_mean_pool": global_mean_pool, "global_add_pool": global_add_pool,
         "global_max_pool": global_max_pool}


# ------------------------------------------------------------------------------------------------
# K2/K3 — fused CGConv
# ------------------------------------------------------------------------------------------------
def _rup(a, b):
    return (a + b - 1) // b * b


# bench.py sets this to {"fwd": [], "bwd": [], "bwd_node": [], "bwd_grads": []} to collect (start, end) HIP events recorded
# on the launch stream around the conv kernels (K2; K3 = edge pass + node kernel + gradient assembly); None = no events.
KERNEL_EVENTS = None


def _launch_timed(key, fn):
    ev = KERNEL_EVENTS
    if ev is None or key not in ev:
        return fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    rc = fn()
    b.record()
    ev[key].append((a, b))
    return rc


class ZeroArena:
    """One zero-filled scratch per training step for the kernels' small accumulators (BatchNorm sums, the conv
    backward's dW partials): a model step needs a dozen of them, and a dozen 5-us fill launches cost more than the
    kernels they serve.  `with ops.zero_arena(device):` around forward + backward zero-fills ONE buffer and hands out
    views; outside of it (or when it is full) zeros() falls back to torch.zeros.  Only for tensors that die with the
    step — nothing that autograd may hand over as a parameter gradient."""

    def __init__(self, device, nbytes=4 << 20):
        self.buf = torch.empty(nbytes // 4, dtype=torch.float32, device=device)
        self.off = 0

    def reset(self):
        self.buf.zero_()
        self.off = 0

    def take(self, shape):
        n = 1
        for d in shape:
            n *= int(d)
        n_al = (n + 63) & ~63                       # 256-byte granules keep every view 16-byte aligned
        if self.off + n_al > self.buf.numel():
            return None
        t = self.buf[self.off:self.off + n].view(*shape)
        self.off += n_al
        return t


_ARENA = None

# Weight-gradient accumulators of the dense layers (the TN GEMM adds into zero-filled [out, in] + [out] buffers): a model
# with dozens of Linear layers would launch dozens of 3-us fills per step.  The model's forward opens ONE freshly
# allocated, zero-filled buffer per step (new_grad_arena) and the backward passes carve their accumulators out of it.
# Unlike the ZeroArena this memory is never reused: the slices become the parameters' .grad tensors and live as long as
# autograd / the optimizer keeps them.
_GRAD_ARENA = None


def new_grad_arena(device, nfloats):
    global _GRAD_ARENA
    _GRAD_ARENA = [torch.zeros(int(nfloats), dtype=torch.float32, device=device), 0]


def _zeros_grad(n, device):
    a = _GRAD_ARENA
    n_al = (int(n) + 63) & ~63
    if a is not None and a[0].device == device and a[1] + n_al <= a[0].numel():
        t = a[0][a[1]:a[1] + int(n)]
        a[1] += n_al
        return t
    return torch.zeros(int(n), dtype=torch.float32, device=device)


class zero_arena:
    def __init__(self, device, nbytes=4 << 20):
        self.key = (torch.device(device), nbytes)

    _cache = {}

    def __enter__(self):
        global _ARENA
        a = zero_arena._cache.get(self.key)
        if a is None:
            a = zero_arena._cache[self.key] = ZeroArena(*self.key)
        a.reset()
        self.prev, _ARENA = _ARENA, a
        return a

    def __exit__(self, *exc):
        global _ARENA
        _ARENA = self.prev
        return False


def _zeros_step(shape, device):
    """fp32 zeros that live no longer than the current step (see ZeroArena)."""
    a = _ARENA
    if a is not None and a.buf.device == device:
        t = a.take(shape)
        if t is not None:
            return t
    return torch.zeros(shape, dtype=torch.float32, device=device)


_WS = {}


def _workspace(device, nbytes):
    """Per-device scratch for the kernels' work counters (the library zeroes what it uses on the stream; launches on one
    stream are ordered, so the layers of a model share it)."""
    key = _stream_key(device)
    t = _WS.get(key)
    if t is None or t.numel() < nbytes:
        t = _WS[key] = torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device=device)
    return t


_TN_SCRATCH = True     # partial sums of the streaming TN products through a scratch buffer + reduce launch instead of atomics
_TNS = {}


_TN_SCRATCH_MIN_ROWS = 4096      # (measured, tools/bench_dense.py: atomics win at 2.6 k rows — 8.2 vs 10.8 us —, the scratch form from 8 k — 13.8 vs 17.8)
# rows from which a bf16 dense layer (forward, dX, the one-pass backward, the TN weight gradient) takes the streaming HIP kernels
# instead of the library's GEMMs
_DENSE_MIN_ROWS = 64        # (1024 until round 6: at ~100 graph rows — the reference's batch size — the library's GEMMs cost 11-12 us each against 5-6)


def _tn_scratch(device, rows=None):
    """Per device and stream: mdl_tn_scratch_bytes() bytes for the _ex forms of the TN products (launches on one stream are
    ordered, so every layer shares it; allocated once — before any HIP-graph capture, by the warm-up steps).  None (= atomics
    from the few workgroups there are) for a product over few rows: at the reference's batch size the reduce launch costs more
    than the handful of atomics it replaces."""
    if not _TN_SCRATCH or (rows is not None and rows < _TN_SCRATCH_MIN_ROWS):
        return None
    key = _stream_key(device)
    t = _TNS.get(key)
    if t is None:
        t = _TNS[key] = torch.empty(lib().mdl_tn_scratch_bytes(), dtype=torch.uint8, device=device)
    return t


def _gemm_tn(a, lda, M, y, ldy, act, b, ldb, K, c, colsum, N, flags, device):
    """mdl_gemm_tn / _colsum / _act in their scratch form (c [M, K] += (a .* act'(y))^T b, colsum += column sums)"""
    return lib().mdl_gemm_tn_ex(ptr(a), lda, M, ptr(y), ldy, act, ptr(b), ldb, K, ptr(c), ptr(colsum), ptr(_tn_scratch(device, N)), N, flags,
                                stream())


# Deterministic mode (include/mdl_hip.h, MDL_DETERMINISTIC): the kernels that combine per-workgroup partial sums with
# floating-point atomics — the CGConv backward edge pass and node kernel, the TN GEMM, the BatchNorm sums, the fused head —
# are launched in a shape in which every sum gets its terms from ONE wave in program order: bit-reproducible from run to run,
# a few hundred times slower.  For HIP-vs-HIP regression checks (graph replay vs eager, padded rows, data-parallel exchange);
# `with ops.deterministic():` or `ops.configure(deterministic=True)` (neither the library nor the package reads the environment).
_DET = False


def set_deterministic(on=True):
    global _DET
    prev, _DET = _DET, bool(on)
    return prev


class deterministic:
    def __init__(self, on=True):
        self.on = on

    def __enter__(self):
        self.prev = set_deterministic(self.on)
        return self

    def __exit__(self, *exc):
        set_deterministic(self.prev)
        return False


# Dispatch options.  Defaults are the measured-best paths; there is NO environment variable behind any of them (round 6): a
# caller that wants another path says so with ops.configure(name=value, ...) — bench.py's `--ops name=value` for A/B runs.
# name -> (module attribute, what it selects)
OPTIONS = {
    "deterministic": ("_DET", "bit-reproducible launch shapes of every atomically accumulating kernel (slow; HIP-vs-HIP tests)"),
    "gmr_dw": ("_GMR_DW", "CFConv backward: dh and dw from one walk over the by-source CSR"),
    "balance": ("_BALANCE", "cost-balanced node ranges for the edge-per-lane CGConv backward (E >= 4e5)"),
    "pad128": ("_PAD128", "C in (96, 128): static 128-channel CGConv kernels on zero-padded rows"),
    "rsrc16": ("_RSRC16", "by-source sums of the CGConv backward in bf16 (packed atomics)"),
    "cfconv_fused": ("_CFCONV_FUSED", "K4: the fused CFConv forward"),
    "cfconv_recompute": ("_CFCONV_RECOMPUTE", "K4b: CFConv backward with the filter recomputed (no per-edge activations)"),
    "tn_colsum": ("_TN_COLSUM", "bias gradients out of the TN GEMM"),
    "dense_bwd": ("_DENSE_BWD", "dX + dW + db of a tall dense layer in one pass"),
    "dense_bwd_wide": ("_DENSE_BWD_WIDE", "... also when both widths exceed 128"),
    "mlp_head": ("_MLP_HEAD", "post-FC head as one launch per direction"),
    "linear_wide": ("_LINEAR_WIDE", "NNConv's Y = x W2r on the streaming kernel"),
    "set2set_fused": ("_SET2SET_FUSED", "Set2Set readout: all processing steps in one launch per direction (off: torch's LSTM + the composed attention)"),
    "tn_scratch": ("_TN_SCRATCH", "weight-gradient blocks of the TN products as plain stores + a reduce launch (off: atomics from every workgroup)"),
}


def configure(**kw):
    """Set dispatch options (see OPTIONS); returns the previous values of the ones given.  Unknown names raise."""
    prev = {}
    g = globals()
    for k, v in kw.items():
        if k not in OPTIONS:
            raise MdlError("ops.configure: unknown option %r (known: %s)" % (k, ", ".join(sorted(OPTIONS))))
        attr = OPTIONS[k][0]
        prev[k] = g[attr]
        g[attr] = bool(v)
    return prev


def options():
    """current value of every dispatch option"""
    return {k: globals()[a] for k, (a, _) in OPTIONS.items()}


def _dflag():
    return _lib.MDL_DETERMINISTIC if _DET else 0


# Which backward edge pass ops.cgconv asks for where both exist (bf16, C = 64, bf16 by-source sums): None = the library's
# edge-count heuristic (kernel 2 from 4e5 edges), "per_wave" / "edge_lane" force one (tests, A/B).
K3_VARIANT = None


def _k3flag():
    return {None: 0, "per_wave": _lib.MDL_K3_PER_WAVE, "edge_lane": _lib.MDL_K3_EDGE_LANE}[K3_VARIANT]


def last_k3():
    """1 per-wave kernel, 2 edge-per-lane kernel 2, 3 per-wave kernel in its deterministic shape (mdl_debug_last_k3)"""
    return int(lib().mdl_debug_last_k3())


_GMR_DW = True          # CFConv backward: dh and dw from one walk over the by-source CSR
_BALANCE = True     # cost-balanced node ranges for the edge-per-lane backward
_PAD128 = True      # C in (96, 128): static 128-channel kernels on zero-padded rows
# By-source sums of the CGConv backward in bf16, accumulated with packed bf16 atomics (mdl_cgconv_bwd_h / mdl_cgconv_bwd_node_h;
# bf16 mode, C in {32, 64, 128}, G = 50): half the atomic operations and bytes of the fp32 buffer; a source row is rounded to bf16
# once per window flush (1-3 partial sums per node).  ops.configure(rsrc16=False) restores the fp32 buffer.
_RSRC16 = True


# r_src (by-source sums of the CGConv backward: fp32 [N, 2*Cp], accumulated with atomics) must start at zero: 107 MB per
# layer at the bench batch, i.e. a 15-22 us fill launch in front of every edge pass.  Its only reader, the node kernel,
# can hand it back zeroed (mdl_cgconv_bwd_node_z), so eager steps keep ONE buffer per device and stream for all layers and
# steps.  `dirty` covers an exception between the two launches; captured graphs keep their own zero-filled tensors.
_RSRC = {}


_RSRC_CAP = {}


def _take_rsrc(nfloats, device):
    if torch.cuda.is_current_stream_capturing():
        # A captured step adopts the buffer its warm-up iterations left behind (training.GraphedStep runs the step eagerly on a
        # side stream, synchronises, then captures): allocated outside the capture, zero on entry, handed back zeroed by the
        # node kernel at the end of every layer — so every replay finds it zero, and the four zero fills per step
        # (53 MB each at the bench batch) that a fresh tensor per layer cost are gone.  The buffer leaves the eager table for
        # good (the graph owns its address); without a clean candidate the caller falls back to a fresh zero-filled tensor.
        # Every adopted buffer stays referenced for the life of the process (a LIST per device): its address is baked into the
        # graph that adopted it, so a later, larger capture must not drop the last reference to it (the allocator would hand the
        # memory out again and a replay of the earlier graph would zero-fill and add into somebody else's tensor).  A buffer
        # whose dirty flag is set (an exception between an edge pass and its node kernel) is never handed to a capture.
        owned = _RSRC_CAP.setdefault(device.index, [])
        for ent in owned:
            if ent[0].numel() >= nfloats and not ent[1]:
                return ent
        cand = [k for k, v in _RSRC.items() if k[0] == device.index and not v[1] and v[0].numel() >= nfloats]
        if not cand:
            return None
        ent = _RSRC.pop(max(cand, key=lambda k: _RSRC[k][0].numel()))
        owned.append(ent)
        return ent
    key = _stream_key(device)
    ent = _RSRC.get(key)
    if ent is None or ent[0].numel() < nfloats or ent[1]:
        ent = _RSRC[key] = [torch.zeros(int(nfloats), dtype=torch.float32, device=device), False]
    return ent


class _CGConvFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, edge_attr, w_f, b_f, w_s, b_s, csr, aggr, packed=None, split=False, d_norm=None, rbf=None):
        require_hip(x, edge_attr, w_f, w_s)
        if edge_attr.dtype != x.dtype:
            raise MdlError("cgconv: x (%s) and edge_attr (%s) must share a dtype" % (x.dtype, edge_attr.dtype))
        x, edge_attr = x.contiguous(), edge_attr.contiguous()
        N, C = x.shape
        E, G = edge_attr.shape
        if csr.N != N or csr.E != E:
            raise MdlError("cgconv: CSR (%d nodes, %d edges) does not match x/edge_attr (%d, %d)" % (csr.N, csr.E, N, E))
        dt = dtype_code(x)
        L = lib()
        # split-bf16 products on fp32 storage (MDL_SPLIT_BF16, the "bf16x3" parity mode): where the kernels have the shape
        # for it (C = 64, G = 50, CSR-ordered edge features); everything else of an fp32 tensor runs the exact form
        # (C = 64; C in (96, 128]: the static 128-channel kernels on zero-padded rows — the reference's default width 100)
        sp = _lib.MDL_SPLIT_BF16 if (split and dt == _lib.MDL_F32 and G == 50 and E > 0 and not _DET
                                     and ((C == 64 and x.data_ptr() % 16 == 0) or (_PAD128 and 96 < C <= 128))) else 0
        ctx.split = sp
        wf32, ws32, bf32, bs32 = _f32c(w_f), _f32c(w_s), _f32c(b_f), _f32c(b_s)
        nbytes = L.mdl_cgconv_wpack_bytes(C, G, dt | sp)
        if nbytes == 0:
            raise MdlError("cgconv: unsupported C=%d G=%d" % (C, G))
        # widths between 97 and 127 (the reference's default dim1 = 100, config.yml:123) run the static 128-channel kernels on
        # zero-padded rows: the packed weights already have that layout (rows / K columns past C are zeros), so the padded
        # output columns hold the constant sigmoid(0) * softplus(0) and are cut off again; their gradients are zeros
        Ck = C
        if _PAD128 and (dt == _lib.MDL_BF16 or sp) and G == 50 and 96 < C < 128 and (csr.eperm is None or sp) and E > 0:
            Ck = 128
            x = torch.nn.functional.pad(x, (0, Ck - C))
        use_packed = packed is not None and packed[3] == (C, G, dt)
        wn_t = None
        if use_packed:
            wpack, bpack, wn_t = packed[:3]               # packed with the model's other layers (cgconv_prepack): no launch here
        elif dt == _lib.MDL_BF16 and (C in (32, 64) or Ck == 128) and any(ctx.needs_input_grad):
            # a training step on the K3c shapes packs the backward node kernel's operand in the same launch
            wpack = torch.empty(nbytes, dtype=torch.uint8, device=x.device)
            bpack = torch.empty(2 * _rup(C, 32), dtype=torch.float32, device=x.device)
            wn_t = torch.empty((C, 4 * _rup(C, 32)), dtype=torch.bfloat16, device=x.device)
            check(L.mdl_cgconv_pack_weights_node(ptr(wf32), ptr(bf32), ptr(ws32), ptr(bs32), C, G, ptr(wpack), ptr(bpack),
                                                 ptr(wn_t), dt, stream()), "mdl_cgconv_pack_weights_node")
        else:
            wpack, bpack = _plain_pack(wf32, bf32, ws32, bs32, C, G, dt | sp, x.device, nbytes)
        ctx.wn_t = wn_t
        out = torch.empty_like(x)
        edge_attr = csr.sorted_attr(edge_attr)          # CSR order: the kernels never go through eperm
        args = _lib.cg_args(dtype=dt, flags=sp, aggr=aggr, N=N, E=E, C=Ck, G=G, x=x, edge_attr=edge_attr, rowptr=csr.rowptr, src=csr.src,
                            tgt=csr.tgt, wpack=wpack, bpack=bpack, out=out)
        check(_launch_timed("fwd", lambda: L.mdl_cgconv_fwd_ex(args, stream())), "mdl_cgconv_fwd_ex")
        # (d_norm, rbf): the edge features are rbf_expand(d_norm) — the backward then returns dL/dd_norm from the fused distance
        # epilogue of the edge-gradient kernel (mdl_cgconv_bwd_edge) instead of an [E, G] gradient
        dist_saved = () if d_norm is None else (d_norm.detach().contiguous(), rbf[0].contiguous())
        ctx.save_for_backward(x, edge_attr, wf32, ws32, wpack, bpack, *dist_saved)
        ctx.rbf_coeff = None if d_norm is None else float(rbf[1])
        ctx.bias32 = (bf32, bs32)
        ctx.csr, ctx.aggr, ctx.has_bias = csr, aggr, (b_f is not None, b_s is not None)
        ctx.wdtypes = (w_f.dtype, w_s.dtype)
        ctx.C = C
        return out if Ck == C else out[:, :C].contiguous()

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        """First order only (once_differentiable: a second differentiation raises).  The gradients of x and the weights are the
        launches they always were; a gradient w.r.t. edge_attr (general epilogue, caller's edge order and dtype) or w.r.t. the
        expanded distance (fused epilogue) costs one launch of the edge-gradient kernel on top."""
        need_de = ctx.needs_input_grad[1]
        need_dd = len(ctx.needs_input_grad) > 10 and ctx.needs_input_grad[10] and ctx.rbf_coeff is not None
        de, dd = _cgconv_edge_grads(ctx, g, need_de, need_dd) if (need_de or need_dd) else (None, None)
        grads = _CGConvFn._backward_main(ctx, g)
        return grads[:1] + (de,) + grads[2:] + (dd, None)

    @staticmethod
    def _backward_main(ctx, g):
        x, edge_attr, wf32, ws32, wpack, bpack = ctx.saved_tensors[:6]
        csr = ctx.csr
        N, Ck = x.shape                                   # Ck: the width the kernels ran at (128 for a padded layer)
        C = ctx.C
        E, G = edge_attr.shape
        Cp, GP = _rup(C, 32), _rup(G, 64)
        g = g.contiguous()
        dt = dtype_code(x)
        xk, gk = x, g
        if Ck != C:
            gk = torch.nn.functional.pad(g, (0, Ck - C))
            x = x[:, :C]                                  # (the node-level part below works on the true width)
        r_tgt = torch.empty((N, 2 * Cp), dtype=x.dtype, device=x.device)          # by-target sums, compute dtype
        sp = ctx.split
        node_x3 = bool(sp) and dt == _lib.MDL_F32 and C == 64                  # split-product node kernel (fp32 storage)
        node_hip = (dt == _lib.MDL_BF16 and C == Cp and C in (32, 64)) or node_x3   # K3c consumes r_tgt / r_src
        rs16 = (_RSRC16 and dt == _lib.MDL_BF16 and (node_hip or Ck == 128) and G == 50 and E > 0
                and x.data_ptr() % 16 == 0 and edge_attr.data_ptr() % 4 == 0)
        nrs = N * 2 * Cp // 2 if rs16 else N * 2 * Cp                         # fp32 words of the by-source buffer
        keep = _take_rsrc(nrs, x.device) if node_hip else None
        if keep is not None:
            r_src, keep[1] = keep[0][:nrs], True
            r_src = r_src.view(torch.bfloat16).view(N, 2 * Cp) if rs16 else r_src.view(N, 2 * Cp)
        else:
            r_src = torch.zeros((N, 2 * Cp), dtype=torch.bfloat16 if rs16 else torch.float32, device=x.device)
        small = _zeros_step((2 * Cp * GP + 2 * Cp + 4 * Cp * C,), x.device)
        dwe = small[:2 * Cp * GP].view(2 * Cp, GP)
        db = small[2 * Cp * GP:2 * Cp * GP + 2 * Cp]
        dwn = small[2 * Cp * GP + 2 * Cp:].view(4 * Cp, C)
        ws = _workspace(x.device, lib().mdl_cgconv_workspace_bytes(N, E, C, G, dt))
        fl = _dflag()
        # node ranges of equal COST (far sources make a tile dearer): one prefix per batch, shared by all layers
        bal = csr.balance() if (rs16 and _BALANCE and E >= 400000 and not fl) else None
        eargs = _lib.cg_args(dtype=dt, flags=fl | (_k3flag() if rs16 else 0) | sp, aggr=ctx.aggr, N=N, E=E, C=Ck, G=G, x=xk, edge_attr=edge_attr,
                             rowptr=csr.rowptr, src=csr.src, tgt=csr.tgt, wpack=wpack, bpack=bpack, grad_out=gk, r_tgt=r_tgt, r_src=r_src,
                             r_src_dtype=_lib.MDL_BF16 if rs16 else _lib.MDL_F32, dwe=dwe, db=db, workspace=ws,
                             workspace_bytes=ws.numel(), balance=bal)
        check(_launch_timed("bwd", lambda: lib().mdl_cgconv_bwd_ex(eargs, stream())), "mdl_cgconv_bwd_ex")
        # node-level dense part: rows of Wn / dWn = (f_tgt, s_tgt, f_src, s_src)
        if node_hip:
            wn_t = _node_weights(ctx, C, Cp, torch.float32 if node_x3 else torch.bfloat16, x.device, wf32, ws32)
            dx = torch.empty_like(x)
            nargs = _lib.cg_node_args(dtype=dt, flags=fl | (sp if node_x3 else 0), zero_src=1 if keep is not None else 0, N=N, C=C,
                                      r_src_dtype=_lib.MDL_BF16 if rs16 else _lib.MDL_F32, x=x, grad_out=g, r_tgt=r_tgt, r_src=r_src,
                                      wn_t=wn_t, dx=dx, dwn=dwn)
            check(_launch_timed("bwd_node", lambda: lib().mdl_cgconv_bwd_node_ex(nargs, stream())), "mdl_cgconv_bwd_node_ex")
            if keep is not None:
                keep[1] = False                                                                     # handed back zeroed
            dW_f, db_f, dW_s, db_s = _assemble_grads(ctx, dwn, dwe, db, C, G, x.device, timed=True)
        elif dt == _lib.MDL_BF16 and Cp == 128 and C % 2 == 0 and N > 0:
            # wide layers (C = 100 / 128): the same products on the streaming kernels.  r_tgt / r_src keep their padded
            # [N, 2 Cp] layout (padded columns are exact zeros), so  dx = g + r_tgt Wn_t + r_src Wn_s  is two library GEMMs on
            # zero-padded weights (no gather / cat of the four column blocks) and  dWn = [r_tgt | r_src]^T x  four TN-GEMM
            # launches (128 rows each) into the [4 Cp, C] layout mdl_cgconv_assemble_grads reads — the library's
            # (4C x N)(N x C) form of that contraction ran 531 us per layer on a 64x64x256 macro tile
            rs_b = r_src.to(torch.bfloat16)
            # Wn^T [C, 4 Cp] (columns f_tgt | s_tgt | f_src | s_src, zero-padded to Cp each) comes packed with the forward's weights
            # (one launch for all layers: cgconv_prepack) — round 6; before, the two zero-padded operands were built here with
            # eight fill / slice-copy / cast launches per layer
            wn_t = _node_weights(ctx, C, Cp, torch.bfloat16, x.device, wf32, ws32)
            dx = torch.addmm(g, r_tgt, wn_t[:, :2 * Cp].t())
            dx.addmm_(rs_b, wn_t[:, 2 * Cp:].t())
            xc = x.contiguous()
            for blk, r in enumerate((r_tgt[:, :Cp], r_tgt[:, Cp:], rs_b[:, :Cp], rs_b[:, Cp:])):
                check(_gemm_tn(r, r.stride(0), Cp, None, 0, 0, xc, xc.stride(0), C, dwn[blk * Cp:(blk + 1) * Cp], None, N, dt | fl,
                               x.device), "mdl_gemm_tn")
            dW_f, db_f, dW_s, db_s = _assemble_grads(ctx, dwn, dwe, db, C, G, x.device, timed=False)
        else:
            Wn = torch.cat([wf32[:, :C], ws32[:, :C], wf32[:, C:2 * C], ws32[:, C:2 * C]], dim=0)      # [4C, C]
            rt = r_tgt.view(N, 2, Cp)[:, :, :C]                                                        # library GEMMs
            rs = r_src.view(N, 2, Cp)[:, :, :C]
            cd = torch.float32 if dt == _lib.MDL_F32 else torch.bfloat16
            R = torch.cat([rt[:, 0], rt[:, 1], rs[:, 0], rs[:, 1]], dim=1).to(cd)                      # [N, 4C]
            dx = torch.addmm(g, R, Wn.to(cd))
            dWn = torch.mm(R.t(), x).float()                                                           # [4C, C]
            dW_f = torch.cat([dWn[0:C], dWn[2 * C:3 * C], dwe[:C, :G]], dim=1)
            dW_s = torch.cat([dWn[C:2 * C], dWn[3 * C:4 * C], dwe[Cp:Cp + C, :G]], dim=1)
            db_f = db[:C].clone() if ctx.has_bias[0] else None
            db_s = db[Cp:Cp + C].clone() if ctx.has_bias[1] else None
        return dx, None, dW_f.to(ctx.wdtypes[0]), db_f, dW_s.to(ctx.wdtypes[1]), db_s, None, None, None, None


def _node_weights(ctx, C, Cp, dtype, device, wf32, ws32):
    """Wn^T [C, 4 Cp] (columns f_tgt | s_tgt | f_src | s_src, zero-padded to Cp each) of the backward's node-level products:
    what the forward (or cgconv_prepack) packed with its own weights, or packed now"""
    wn_t, ctx.wn_t = ctx.wn_t, None
    if wn_t is None:
        wn_t = torch.empty((C, 4 * Cp), dtype=dtype, device=device)
        check(lib().mdl_cgconv_pack_node_weights(ptr(wf32), ptr(ws32), C, wf32.shape[1] - 2 * C, ptr(wn_t), dtype_code(wn_t), stream()),
              "mdl_cgconv_pack_node_weights")
    return wn_t


def _assemble_grads(ctx, dwn, dwe, db, C, G, device, timed):
    """(dW_f, db_f, dW_s, db_s) fp32 from the kernels' staging buffers (mdl_cgconv_assemble_grads)"""
    dW_f = torch.empty((C, 2 * C + G), dtype=torch.float32, device=device)
    dW_s = torch.empty_like(dW_f)
    db_f = torch.empty(C, dtype=torch.float32, device=device) if ctx.has_bias[0] else None
    db_s = torch.empty(C, dtype=torch.float32, device=device) if ctx.has_bias[1] else None
    launch = lambda: lib().mdl_cgconv_assemble_grads(ptr(dwn), ptr(dwe), ptr(db), C, G, ptr(dW_f), ptr(dW_s), ptr(db_f), ptr(db_s), stream())
    check(_launch_timed("bwd_grads", launch) if timed else launch(), "mdl_cgconv_assemble_grads")
    return dW_f, db_f, dW_s, db_s


def cgconv_prepack(convs, x_dtype, device, want_node=True):
    """The packed weights of several CGConv layers of equal shape in ONE launch (mdl_cgconv_pack_weights_multi): a list of
    (wpack, bpack, wn_t, key) to hand to cgconv(..., packed=...), or None when the layers do not share a shape / the fast
    path does not apply.  A model calls it once per forward: the layers' weights are all known before the first one runs."""
    import ctypes
    if len(convs) < 2 or len(convs) > 16 or device.type != "cuda":
        return None
    C, G = convs[0].channels, convs[0].dim
    dt = _lib.MDL_BF16 if x_dtype == torch.bfloat16 else _lib.MDL_F32
    if any(c.channels != C or c.dim != G or c.lin_f.weight.dtype != torch.float32 or not c.lin_f.weight.is_contiguous()
           or not c.lin_s.weight.is_contiguous() or (c.lin_f.bias is None) != (convs[0].lin_f.bias is None) for c in convs):
        return None
    if not (dt == _lib.MDL_BF16 and (C in (32, 64) or (_PAD128 and G == 50 and 96 < C < 128))):
        return None
    L = lib()
    nbytes = L.mdl_cgconv_wpack_bytes(C, G, dt)
    if nbytes == 0:
        return None
    n = len(convs)
    wbuf = torch.empty((n, nbytes), dtype=torch.uint8, device=device)
    bbuf = torch.empty((n, 2 * _rup(C, 32)), dtype=torch.float32, device=device)
    nbuf = torch.empty((n, C, 4 * _rup(C, 32)), dtype=torch.bfloat16, device=device) if want_node else None
    tab = lambda ts: (ctypes.c_void_p * n)(*[None if t is None else t.data_ptr() for t in ts])
    has_b = convs[0].lin_f.bias is not None
    check(L.mdl_cgconv_pack_weights_multi(
        n, tab([c.lin_f.weight.detach() for c in convs]), tab([c.lin_f.bias.detach() for c in convs]) if has_b else None,
        tab([c.lin_s.weight.detach() for c in convs]), tab([c.lin_s.bias.detach() for c in convs]) if has_b else None, C, G,
        tab(list(wbuf)), tab(list(bbuf)), tab(list(nbuf)) if want_node else None, dt, stream()), "mdl_cgconv_pack_weights_multi")
    return [(wbuf[k], bbuf[k], nbuf[k] if want_node else None, (C, G, dt)) for k in range(n)]


def cgconv(x, edge_index, edge_attr, w_f, b_f, w_s, b_s, aggr="mean", csr=None, packed=None, split=False, dist=None):
    """CGConv forward.  x [N,C], edge_index [2,E], edge_attr [E,G]; returns [N,C].  Differentiable (first order) in
    x, the weights and edge_attr, like upstream's operator; the edge_attr gradient comes back in the caller's edge order and in
    edge_attr's dtype from one extra launch (csrc/cgconv_de.hip), and only when edge_attr requires it.
    dist = (d_norm [E] fp32, offsets [G] fp32, coeff): a promise that edge_attr = rbf_expand(d_norm) on these centres (detached:
    edge_attr itself carries no gradient).  The backward then hands d_norm its gradient from the kernel's fused distance epilogue,
    and no [E, G] gradient is ever stored.  Under split=True ("bf16x3") the edge-gradient kernel runs its exact fp32 form."""
    if aggr not in ("mean", "add", "sum"):
        raise MdlError("cgconv: aggr must be mean or add")
    if csr is None:
        csr = csr_for(edge_index, x.shape[0])
    if dist is None:
        return _CGConvFn.apply(x, edge_attr, w_f, b_f, w_s, b_s, csr, _lib.REDUCE[aggr], packed, split)
    d_norm, offsets, coeff = _check_dist("cgconv", dist, edge_attr, "edge_attr")
    return _CGConvFn.apply(x, edge_attr, w_f, b_f, w_s, b_s, csr, _lib.REDUCE[aggr], packed, split, d_norm, (offsets.float(), float(coeff)))


def _check_dist(name, dist, edge_attr, what):
    """dist = (d_norm, offsets, coeff) of cgconv / cfconv, validated against the edge features (`what`: their name in the message)"""
    d_norm, offsets, coeff = dist
    require_hip(d_norm, offsets)
    if d_norm.dtype != torch.float32 or d_norm.numel() != edge_attr.shape[0] or offsets.numel() != edge_attr.shape[1]:
        raise MdlError("%s: dist = (d_norm [E] float32, offsets [G], coeff) must match %s %s" % (name, what, tuple(edge_attr.shape)))
    return d_norm, offsets, coeff


def _dist_grad_inputs(name, x, edge_index, d_norm, csr, start, stop, resolution, width, edge_attr, out):
    """What the two *_dist_grad functions share: (csr, offsets [G], d_norm in CSR order, edge features in CSR order and x's dtype —
    the caller's edge_attr, or the expansion of d_norm)."""
    if csr is None:
        csr = csr_for(edge_index, x.shape[0])
    if d_norm.dtype != torch.float32 or d_norm.numel() != csr.E or csr.N != x.shape[0]:
        raise MdlError("%s: d_norm must be [E] float32 over the CSR's %d edges" % (name, csr.E))
    if out is not None and csr.eperm is not None:
        raise MdlError("%s: out= needs an edge list in CSR (target-sorted) order" % name)
    offsets = rbf_offsets(start, stop, resolution, x.device)
    d_sorted = _sort_edges(d_norm, csr).contiguous()
    if edge_attr is None:
        ea = rbf_expand(d_sorted.detach(), start, stop, resolution, width, out_dtype=x.dtype, offsets=offsets)
    else:
        ea = csr.sorted_attr(edge_attr.detach().contiguous())
    return csr, offsets, d_sorted, ea


def _bwd_edge_launch(x, ea_sorted, csr, wpack, bpack, g, aggr, C, G, de=None, d_sorted=None, offsets=None, coeff=0.0, scale=1.0, dd=None):
    """mdl_cgconv_bwd_edge on CSR-ordered operands: de [E, G] (general epilogue) or dd [E] += (distance epilogue)."""
    check(_launch_timed("bwd_edge", lambda: lib().mdl_cgconv_bwd_edge(
        ptr(x), ptr(ea_sorted), ptr(csr.rowptr), ptr(csr.src), ptr(csr.tgt), ptr(wpack), ptr(bpack), ptr(g), x.shape[0], ea_sorted.shape[0],
        C, G, aggr, dtype_code(x), ptr(de), ptr(d_sorted), ptr(offsets), float(coeff), float(scale), ptr(dd), stream())),
        "mdl_cgconv_bwd_edge")


def _plain_pack(wf32, bf32, ws32, bs32, C, G, dt, device, nbytes=None):
    """(wpack, bpack) of one layer by mdl_cgconv_pack_weights; nbytes: mdl_cgconv_wpack_bytes(C, G, dt) where the caller has it"""
    wpack = torch.empty(lib().mdl_cgconv_wpack_bytes(C, G, dt) if nbytes is None else nbytes, dtype=torch.uint8, device=device)
    bpack = torch.empty(2 * _rup(C, 32), dtype=torch.float32, device=device)
    check(lib().mdl_cgconv_pack_weights(ptr(wf32), ptr(bf32), ptr(ws32), ptr(bs32), C, G, ptr(wpack), ptr(bpack), dt, stream()),
          "mdl_cgconv_pack_weights")
    return wpack, bpack


def _unsort_edges(t, csr):
    """a per-edge tensor in CSR order -> the caller's edge order"""
    if csr.eperm is None:
        return t
    out = torch.empty_like(t)
    out[csr.eperm.long()] = t
    return out


def _cgconv_edge_grads(ctx, g, need_de, need_dd):
    """The per-edge gradients of one CGConv layer (see _CGConvFn.backward): (de or None, dd or None) in the caller's edge order."""
    saved = ctx.saved_tensors
    x, edge_attr, wf32, ws32, wpack, bpack = saved[:6]
    csr = ctx.csr
    C = ctx.C
    E, G = edge_attr.shape
    dt = dtype_code(x)
    if x.shape[1] != C:
        x = x[:, :C].contiguous()                         # a padded layer: the edge-gradient kernel runs at the true width
    g = g.contiguous()
    if ctx.split:                                         # bf16x3 layer: exact fp32 form on plainly packed weights
        wpack, bpack = _plain_pack(wf32, ctx.bias32[0], ws32, ctx.bias32[1], C, G, dt, x.device)
    de = dd = None
    if need_de:
        de = (torch.zeros if csr.partial else torch.empty)((E, G), dtype=edge_attr.dtype, device=x.device)
        _bwd_edge_launch(x, edge_attr, csr, wpack, bpack, g, ctx.aggr, C, G, de=de)
        de = _unsort_edges(de, csr)
    if need_dd:
        d_norm, offsets = saved[6], saved[7]
        d_sorted = _sort_edges(d_norm, csr)
        dd = torch.zeros(E, dtype=torch.float32, device=x.device)
        _bwd_edge_launch(x, edge_attr, csr, wpack, bpack, g, ctx.aggr, C, G, d_sorted=d_sorted, offsets=offsets, coeff=ctx.rbf_coeff, dd=dd)
        dd = _unsort_edges(dd, csr)
    return de, dd


def cgconv_dist_grad(x, edge_index, d_norm, w_f, b_f, w_s, b_s, grad_out, aggr="mean", csr=None, start=0.0, stop=1.0, resolution=50,
                     width=0.2, scale=1.0, edge_attr=None, out=None):
    """dL/dd of ONE CGConv layer whose edge features are the Gaussian expansion rbf_expand(d_norm, start, stop, resolution, width)
    in x's dtype, for the output gradient grad_out [N, C]: the fused distance epilogue of the edge-gradient kernel
    (csrc/cgconv_de.hip) —  scale * sum_g de[e, g] * d e[e, g] / d d_norm[e]  per edge, with de kept in registers.
    `scale` is the chain-rule factor of the caller's normalisation (1 / (max - min) for raw distances).  Returns [E] fp32 in the
    caller's edge order; `out` ([E] fp32, CSR-ordered edge lists only) is added into instead, so that the layers of a model
    accumulate in one buffer.  No atomics: bitwise repeatable.  No gradient flows through this call itself."""
    if aggr not in ("mean", "add", "sum"):
        raise MdlError("cgconv_dist_grad: aggr must be mean or add")
    require_hip(x, d_norm, w_f, w_s, grad_out)
    with torch.no_grad():
        C, G, dt = x.shape[1], int(resolution), dtype_code(x)
        if lib().mdl_cgconv_wpack_bytes(C, G, dt) == 0:
            raise MdlError("cgconv_dist_grad: unsupported C=%d G=%d" % (C, G))
        csr, offsets, d_sorted, ea = _dist_grad_inputs("cgconv_dist_grad", x, edge_index, d_norm, csr, start, stop, G, width, edge_attr, out)
        wpack, bpack = _plain_pack(_f32c(w_f), _f32c(b_f), _f32c(w_s), _f32c(b_s), C, G, dt, x.device)
        dd = out if out is not None else torch.zeros(csr.E, dtype=torch.float32, device=x.device)
        _bwd_edge_launch(x.detach().contiguous(), ea, csr, wpack, bpack, grad_out.detach().to(x.dtype).contiguous(), _lib.REDUCE[aggr], C, G,
                         d_sorted=d_sorted, offsets=offsets, coeff=rbf_coeff(start, stop, width), scale=scale, dd=dd)
        return dd if out is not None else _unsort_edges(dd, csr)


# ------------------------------------------------------------------------------------------------
# generic gather / edge-weighted gather-reduce (SchNet CFConv, GCNConv, MEGNet, NNConv building blocks)
# ------------------------------------------------------------------------------------------------
class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, src, index):
        require_hip(src, index)
        src = src.contiguous()
        idx = index.to(torch.int32).contiguous()
        C = src.numel() // max(src.shape[0], 1)
        out = torch.empty((idx.numel(),) + tuple(src.shape[1:]), dtype=src.dtype, device=src.device)
        check(lib().mdl_gather_rows(ptr(src), ptr(idx), ptr(out), idx.numel(), C, dtype_code(src), stream()),
              "mdl_gather_rows")
        ctx.index, ctx.n = index, src.shape[0]
        return out

    @staticmethod
    def backward(ctx, g):
        return scatter(g, ctx.index, 0, ctx.n, "sum"), None


def gather(src, index):
    """src.index_select(0, index) with a HIP forward and a segmented-reduce backward."""
    return _Gather.apply(src, index)


class _GatherMulReduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, h, w, scale, csr, reduce, pre=None):
        # pre: the result, already formed by the fused CFConv forward (cfconv_fused) — this node then only records the graph
        require_hip(h)
        h = h.contiguous()
        N, F = csr.N, h.shape[1]
        if w is not None:
            w = w.contiguous()
            if w.dtype != h.dtype:
                raise MdlError("gather_mul_reduce: h and w must share a dtype")
        if scale is not None:
            scale = scale.float().contiguous()
        if pre is not None:
            out = pre.view_as(pre)
        else:
            out = torch.empty((N, F), dtype=h.dtype, device=h.device)
            check(_launch_timed("gmr_fwd", lambda: lib().mdl_gather_mul_reduce(
                ptr(h), ptr(w), ptr(scale), ptr(csr.rowptr), ptr(csr.src), ptr(csr.eperm), ptr(out), N, F, reduce, dtype_code(h),
                stream())), "mdl_gather_mul_reduce")
        ctx.csr, ctx.reduce = csr, reduce
        ctx.save_for_backward(h, w, scale)
        return out

    @staticmethod
    def backward(ctx, g):
        h, w, scale = ctx.saved_tensors
        csr = ctx.csr
        g = g.contiguous()
        if ctx.reduce == _lib.MDL_MEAN:
            deg = (csr.rowptr[1:] - csr.rowptr[:-1]).clamp(min=1).to(g.dtype)
            g = g / deg.unsqueeze(1)
        dh = dw = None
        if scale is not None and ctx.needs_input_grad[2]:
            # dscale[e] = sum_f g[tgt_e, f] h[src_e, f] w[e, f] (mdl_edge_dot): the cosine cutoff of CFConv as a function of the
            # positions; GCNConv's normalised gather-reduce gets the same gradient for free
            dscale = torch.empty(csr.E, dtype=torch.float32, device=h.device)
            check(lib().mdl_edge_dot(ptr(g), ptr(csr.col), ptr(h), ptr(csr.row), ptr(w), ptr(dscale), csr.E, h.shape[1],
                                     dtype_code(h), stream()), "mdl_edge_dot")
            dh, dw = _gmr_dh_dw(ctx, g, h, w, scale, csr)
            return dh, dw, dscale, None, None, None
        if (w is not None and ctx.needs_input_grad[0] and ctx.needs_input_grad[1] and _GMR_DW and h.dtype == torch.bfloat16
                and h.shape[1] % 2 == 0 and h.shape[1] <= 512 and scale is not None):
            # one walk over the by-source CSR gives both gradients (no mdl_edge_mul pass)
            rowptr_s, col_s, eid_s, _ = csr.transposed()
            dh = torch.empty_like(h)
            # (unused edge slots of a padded static batch belong to no by-source segment: their dw rows must read as zeros)
            dw = (torch.zeros_like if _true_rows_for(w.shape[0]) is not None else torch.empty_like)(w)
            check(lib().mdl_gather_mul_reduce_dw(ptr(g), ptr(w), ptr(scale), ptr(rowptr_s), ptr(col_s), ptr(eid_s), ptr(dh), ptr(h),
                                                 ptr(dw), csr.N, h.shape[1], dtype_code(h), stream()), "mdl_gather_mul_reduce_dw")
            return dh, dw, None, None, None, None
        dh, dw = _gmr_dh_dw(ctx, g, h, w, scale, csr)
        return dh, dw, None, None, None, None


def _gmr_dh_dw(ctx, g, h, w, scale, csr):
    """(dh, dw) of _GatherMulReduce by the two separate launches: the transposed gather-reduce and mdl_edge_mul"""
    dh = dw = None
    if ctx.needs_input_grad[0]:
        rowptr_s, col_s, eid_s, _ = csr.transposed()
        dh = torch.empty_like(h)
        check(lib().mdl_gather_mul_reduce(ptr(g), ptr(w), ptr(scale), ptr(rowptr_s), ptr(col_s), ptr(eid_s),
                                          ptr(dh), csr.N, h.shape[1], _lib.MDL_SUM, dtype_code(h), stream()),
              "mdl_gather_mul_reduce(T)")
    if w is not None and ctx.needs_input_grad[1]:
        dw = torch.empty_like(w)
        check(lib().mdl_edge_mul(ptr(h), ptr(csr.row), ptr(g), ptr(csr.col), ptr(scale), ptr(dw), csr.E,
                                 h.shape[1], dtype_code(h), stream()), "mdl_edge_mul")
    return dh, dw


def gather_mul_reduce(h, csr, w=None, scale=None, reduce="sum", pre=None):
    """out[i] = reduce_{edges k -> i} h[src_k] * w[k] * scale[k]  (w: [E,F], scale: [E], caller's edge order).
    Differentiable in h, w and scale (scale: [E] fp32 from mdl_edge_dot, only when it requires a gradient — SchNet's cutoff as a
    function of the positions; GCNConv's edge normalisation gets the same gradient for free)."""
    return _GatherMulReduce.apply(h, w, scale, csr, _lib.REDUCE[reduce], pre)


# ------------------------------------------------------------------------------------------------
# K4 — the fused CFConv forward (csrc/cfconv.hip): filter network + cutoff + h[src] * W -> segmented sum in one pass
# ------------------------------------------------------------------------------------------------
_CFCONV_FUSED = True
_CFCONV_RECOMPUTE = True
# Forward + backward of the block at E = 1.46 M (profiles/r06d_k4_k4b_forms.txt; K4 and K4b both static at the padded width 96 /
# 128 / 160): F = 64: 864 us recomputing / 696 stored / 748 unfused; 80: 899 / 886 / 952; 100: 1048 / 1076 / 1126; 112: 1055 / 1115 /
# 1175; 128: 1215 / 1313 / 1343; 150: 1254 / 1686 / 1794 — the recomputing backward from the 128-wide instantiation on (it also keeps
# 2 E F s bytes of activations per layer out of memory), stored activations below
_CFCONV_RECOMPUTE_MIN_F = 96


def cfconv_fused_ok(rbf, h, csr, lin_a, lin_b):
    """the fused forward takes (edge features [E, 50] bf16 in CSR order, h [N, F] bf16, the two Linears of the filter network):
    shapes mdl_cfconv_fwd supports AND for which both dense layers would take the fused dense path (the backward is theirs)."""
    if not (_CFCONV_FUSED and rbf.is_cuda and rbf.dtype == torch.bfloat16 and h.dtype == torch.bfloat16 and rbf.dim() == 2
            and h.dim() == 2 and rbf.is_contiguous() and csr.eperm is None and rbf.shape[0] == csr.E):
        return False
    F, G = h.shape[1], rbf.shape[1]
    if tuple(lin_a.weight.shape) != (F, G) or tuple(lin_b.weight.shape) != (F, F):
        return False
    # mdl_cfconv_pack_weights reads both weights and both biases as dense fp32 rows
    for t in (lin_a.weight, lin_b.weight, lin_a.bias, lin_b.bias):
        if t is not None and (t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda):
            return False
    if not lib().mdl_cfconv_supported(F, G, dtype_code(h)):
        return False
    if torch.is_grad_enabled() and (lin_a.weight.requires_grad or lin_b.weight.requires_grad or h.requires_grad):
        # the autograd nodes this forward stands in for: _LinearActTN (ssp, derivative handed down) -> _LinearActTN -> K4a
        return (linear_act_fused_ok(rbf, lin_a.weight, "ssp") and _hip_shape_ok(F, F) and rbf.shape[0] >= _DENSE_MIN_ROWS
                and lin_a.weight.requires_grad and lin_b.weight.requires_grad)
    return True


def cfconv_fused(rbf, cut, h, csr, lin_a, lin_b, want_acts):
    """One launch (plus the weight packing): out [N, F] and, with want_acts, the layer-1 output a1 [E, F] and the filter w [E, F]."""
    require_hip(rbf, h)
    F, G = h.shape[1], rbf.shape[1]
    E, N = csr.E, csr.N
    dev = h.device
    wpack = _cfconv_pack(lin_a.weight, lin_a.bias, lin_b.weight, lin_b.bias, F, G, dev)
    out = torch.empty((N, F), dtype=h.dtype, device=dev)
    a1 = torch.empty((E, F), dtype=h.dtype, device=dev) if want_acts else None
    w = torch.empty((E, F), dtype=h.dtype, device=dev) if want_acts else None
    h = h.contiguous()
    _cfconv_fwd_launch("cfconv_fwd", rbf, cut.float().contiguous(), h, csr.rowptr, csr.src, csr.tgt, wpack, N, E, out, a1, w)
    return out, a1, w


def _cfconv_pack(w1, b1, w2, b2, F, G, device):
    """the filter network's weights (dense fp32 rows) in the layout of the CFConv kernels"""
    wpack = torch.empty(lib().mdl_cfconv_wpack_bytes(), dtype=torch.uint8, device=device)
    check(lib().mdl_cfconv_pack_weights(ptr(w1), ptr(b1), ptr(w2), ptr(b2), F, G, ptr(wpack), stream()), "mdl_cfconv_pack_weights")
    return wpack


def _cfconv_fwd_launch(key, rbf, cut, x, rowptr, src, tgt, wpack, N, E, out, a1=None, w=None):
    """mdl_cfconv_fwd: out[i] = sum over row i of x[src] * W(rbf) * cut.  key "cfconv_fwd": the forward on the by-target CSR
    (a1, w: the per-edge activations, where wanted); "cfconv_bwd_h": the same kernel on the by-source CSR with x = grad_out
    and (rbf, cut) in by-source order, which is dh."""
    F, G = x.shape[1], rbf.shape[1]
    check(_launch_timed(key, lambda: lib().mdl_cfconv_fwd(
        ptr(rbf), ptr(cut), ptr(x), ptr(rowptr), ptr(src), ptr(tgt), ptr(wpack), ptr(out), ptr(a1), ptr(w), N, E, F, G,
        dtype_code(out), stream())), "mdl_cfconv_fwd" if key == "cfconv_fwd" else "mdl_cfconv_fwd(T)")


def _cfconv_param_grads(rbf, cut, h, g, csr, wpack, has_b):
    """(dw1, db1, dw2, db2) of the filter network by mdl_cfconv_bwd_w (the filter is recomputed): fp32 views of one buffer"""
    F, G = h.shape[1], rbf.shape[1]
    buf = torch.zeros(F * G + F * F + 2 * F, dtype=torch.float32, device=h.device)    # (not the step arena: autograd may adopt these views as .grad)
    dw1, dw2 = buf[:F * G].view(F, G), buf[F * G:F * G + F * F].view(F, F)
    db1 = buf[F * G + F * F:F * G + F * F + F] if has_b[0] else None
    db2 = buf[F * G + F * F + F:] if has_b[1] else None
    scratch = torch.empty(lib().mdl_cfconv_bwd_w_scratch_bytes(), dtype=torch.uint8, device=h.device)
    check(_launch_timed("cfconv_bwd_w", lambda: lib().mdl_cfconv_bwd_w(
        ptr(rbf), ptr(cut), ptr(h), ptr(g), ptr(csr.rowptr), ptr(csr.src), ptr(csr.tgt), ptr(wpack), ptr(dw1), ptr(db1),
        ptr(dw2), ptr(db2), ptr(scratch), csr.N, csr.E, F, G, dtype_code(h) | _dflag(), stream())), "mdl_cfconv_bwd_w")
    return dw1, db1, dw2, db2


class BySourceAttrs:
    """(rbf, cut) rows in by-source order for the backward of the recomputing CFConv (K4b): the same for every interaction block
    of a model, so a model makes ONE of these per forward call and hands it to its blocks; the first backward to run gathers
    (one mdl_gather_rows over [E, G] + one over [E]), the others reuse.  Lives exactly as long as the autograd graph of that
    forward — nothing is keyed on tensor identity, so the in-place rewritten buffers of a HIP-graph replay are safe."""

    def __init__(self):
        self._v = None

    def get(self, rbf, cut, eid_s):
        if self._v is None:
            rbf_s = torch.empty_like(rbf)
            check(lib().mdl_gather_rows(ptr(rbf), ptr(eid_s), ptr(rbf_s), eid_s.numel(), rbf.shape[1], dtype_code(rbf), stream()),
                  "mdl_gather_rows")                 # (torch's index_select on [E, 50] bf16 rows: 177 us against 60)
            self._v = (rbf_s, cut.index_select(0, eid_s.long()))
        return self._v


def cfconv_recompute(rbf, cut, h, csr, lin_a, lin_b, cache=None):
    """K4 + K4b: the CFConv aggregation as ONE autograd node that stores nothing per edge (see cfconv_fused_ok for the shapes)."""
    return _CFConv.apply(rbf, cut, h, lin_a.weight, lin_a.bias, lin_b.weight, lin_b.bias, csr, None, None, cache)


# ------------------------------------------------------------------------------------------------
# K4d — CFConv gradients w.r.t. the per-edge inputs (csrc/cfconv_de.hip): forces for SchNet
# ------------------------------------------------------------------------------------------------
# launches of mdl_cfconv_bwd_edge by epilogue (tests assert that the kernel, not the general composition, served a case)
K4D_LAUNCHES = collections.Counter()


def cfconv_edge_ok(rbf, h, w1, w2):
    """mdl_cfconv_bwd_edge takes these operands: bf16 at the shapes of the fused forward, fp32 while the weights fit the LDS"""
    if not (rbf.is_cuda and rbf.dim() == 2 and h.dim() == 2 and rbf.dtype == h.dtype and h.dtype in (torch.float32, torch.bfloat16)):
        return False
    F, G = h.shape[1], rbf.shape[1]
    if tuple(w1.shape) != (F, G) or tuple(w2.shape) != (F, F):
        return False
    return bool(lib().mdl_cfconv_bwd_edge_supported(F, G, dtype_code(h)))


def _cfconv_bwd_edge_launch(rbf_s, cut_s, h, g, csr, wpack, w1, b1, w2, b2, dcut=None, drbf=None, d_sorted=None, offsets=None,
                            coeff=0.0, scale=1.0, dd=None):
    """mdl_cfconv_bwd_edge on CSR-ordered operands"""
    K4D_LAUNCHES["distance" if dd is not None else ("general" if drbf is not None else "dcut")] += 1
    F, G = h.shape[1], rbf_s.shape[1]
    check(_launch_timed("cfconv_bwd_edge", lambda: lib().mdl_cfconv_bwd_edge(
        ptr(rbf_s), ptr(cut_s), ptr(h), ptr(g), ptr(csr.rowptr), ptr(csr.src), ptr(csr.tgt), ptr(wpack), ptr(w1), ptr(b1), ptr(w2),
        ptr(b2), csr.N, csr.E, F, G, dtype_code(h), ptr(dcut), ptr(drbf), ptr(d_sorted), ptr(offsets), float(coeff), float(scale),
        ptr(dd), stream())), "mdl_cfconv_bwd_edge")


def _sort_edges(t, csr):
    return t if csr.eperm is None else t.index_select(0, csr.eperm.long())


def _filter_f32(rbf, w1, b1, w2, b2):
    a = torch.nn.functional.softplus(torch.nn.functional.linear(rbf, w1, b1)) - _LN2
    return torch.nn.functional.linear(a, w2, b2)


class _CFConv(torch.autograd.Function):
    """The CFConv aggregation as ONE autograd node that stores nothing per edge and is differentiable (first order) in h, the
    filter network's parameters and the per-edge inputs.
    forward: bf16 = mdl_cfconv_fwd without activations; fp32 = the filter network + mdl_gather_mul_reduce.  backward: dh by the
    same kernel on the by-source CSR (cache: the model's BySourceAttrs, shared by its blocks), the parameter gradients by
    mdl_cfconv_bwd_w (csrc/cfconv_bwd.hip) — the filter is recomputed in both —, and K4d for the edge inputs that ask: dcut for
    the cutoff, the distance epilogue for d_norm (dist given), the general epilogue for rbf.
    On the training path (cfconv_recompute: bf16, CSR-ordered edges, dense fp32 weights, no gradient on rbf / cut) every
    conversion of the forward is an identity: the launches are the packing, the forward, dh and mdl_cfconv_bwd_w."""

    @staticmethod
    def forward(ctx, rbf, cut, h, w1, b1, w2, b2, csr, d_norm, meta, cache):
        require_hip(rbf, h, cut)
        F, G = h.shape[1], rbf.shape[1]
        bf = h.dtype == torch.bfloat16
        w1f, b1f, w2f, b2f = _f32c(w1), _f32c(b1), _f32c(w2), _f32c(b2)
        wpack = _cfconv_pack(w1f, b1f, w2f, b2f, F, G, h.device) if bf else None
        out = torch.empty((csr.N, F), dtype=h.dtype, device=h.device)
        h = h.contiguous()
        rbf_s = csr.sorted_attr(rbf.contiguous())
        cut_s = _sort_edges(cut.float(), csr).contiguous()
        if bf:
            _cfconv_fwd_launch("cfconv_fwd", rbf_s, cut_s, h, csr.rowptr, csr.src, csr.tgt, wpack, csr.N, csr.E, out)
        else:
            w_s = _filter_f32(rbf_s, w1f, b1f, w2f, b2f).contiguous()
            check(lib().mdl_gather_mul_reduce(ptr(h), ptr(w_s), ptr(cut_s), ptr(csr.rowptr), ptr(csr.src), None, ptr(out), csr.N, F,
                                              _lib.MDL_SUM, dtype_code(h), stream()), "mdl_gather_mul_reduce")
        ctx.csr, ctx.meta, ctx.cache, ctx.has_b = csr, meta, cache, (b1 is not None, b2 is not None)
        ctx.save_for_backward(rbf_s, cut_s, h, wpack, w1f, b1f, w2f, b2f, d_norm)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        rbf_s, cut_s, h, wpack, w1f, b1f, w2f, b2f, d_norm = ctx.saved_tensors
        csr = ctx.csr
        N, E, F, G = csr.N, csr.E, h.shape[1], rbf_s.shape[1]
        bf = h.dtype == torch.bfloat16
        g = g.contiguous()
        need = ctx.needs_input_grad
        drbf = dcut = dh = dw1 = db1 = dw2 = db2 = ddn = None
        if need[2]:
            rowptr_s, col_s, eid_s, src_sorted = csr.transposed()
            # (eid_s numbers the caller's edges; the saved rows are in CSR order: compose with the inverse of eperm)
            if csr.eperm is None:
                pos_s = eid_s
            else:
                inv = _unsort_edges(torch.arange(E, dtype=csr.eperm.dtype, device=h.device), csr)
                pos_s = inv.index_select(0, eid_s.long()).contiguous()
            dh = torch.empty_like(h)
            if bf:
                rbf_t, cut_t = (ctx.cache if ctx.cache is not None else BySourceAttrs()).get(rbf_s, cut_s, pos_s)
                _cfconv_fwd_launch("cfconv_bwd_h", rbf_t, cut_t, g, rowptr_s, col_s, src_sorted, wpack, N, E, dh)
            else:
                w_s = _filter_f32(rbf_s, w1f, b1f, w2f, b2f).contiguous()
                check(lib().mdl_gather_mul_reduce(ptr(g), ptr(w_s), ptr(cut_s), ptr(rowptr_s), ptr(col_s), ptr(pos_s), ptr(dh),
                                                  N, F, _lib.MDL_SUM, dtype_code(h), stream()), "mdl_gather_mul_reduce(T)")
        if need[3] or need[4] or need[5] or need[6]:
            if bf:
                dw1, db1, dw2, db2 = _cfconv_param_grads(rbf_s, cut_s, h, g, csr, wpack, ctx.has_b)
            else:
                # fp32: the filter gradient by mdl_edge_mul, the two dense layers' parameter gradients by the library
                dwf = torch.empty((E, F), dtype=h.dtype, device=h.device)
                check(lib().mdl_edge_mul(ptr(h), ptr(csr.src), ptr(g), ptr(csr.tgt), ptr(cut_s), ptr(dwf), E, F, dtype_code(h), stream()),
                      "mdl_edge_mul")
                if csr.partial:
                    dwf[int(csr.rowptr[-1]):] = 0
                pre = torch.nn.functional.linear(rbf_s, w1f, b1f)
                a = torch.nn.functional.softplus(pre) - _LN2
                dw2, db2 = dwf.t() @ a, (dwf.sum(0) if ctx.has_b[1] else None)
                da = (dwf @ w2f) * torch.sigmoid(pre)
                dw1, db1 = da.t() @ rbf_s, (da.sum(0) if ctx.has_b[0] else None)
        want_dd = d_norm is not None and need[8]
        if need[0] or need[1] or want_dd:
            if need[1]:
                dcut = (torch.zeros if csr.partial else torch.empty)(E, dtype=torch.float32, device=h.device)
            if need[0]:
                drbf = (torch.zeros if csr.partial else torch.empty)((E, G), dtype=rbf_s.dtype, device=h.device)
                _cfconv_bwd_edge_launch(rbf_s, cut_s, h, g, csr, wpack, w1f, b1f, w2f, b2f, dcut=None if want_dd else dcut, drbf=drbf)
                drbf = _unsort_edges(drbf, csr)
            if want_dd:
                offsets, coeff = ctx.meta
                ddn = torch.zeros(E, dtype=torch.float32, device=h.device)
                _cfconv_bwd_edge_launch(rbf_s, cut_s, h, g, csr, wpack, w1f, b1f, w2f, b2f, dcut=dcut, d_sorted=_sort_edges(d_norm, csr).contiguous(),
                                        offsets=offsets, coeff=coeff, dd=ddn)
                ddn = _unsort_edges(ddn, csr)
            elif need[1] and not need[0]:
                _cfconv_bwd_edge_launch(rbf_s, cut_s, h, g, csr, wpack, w1f, b1f, w2f, b2f, dcut=dcut)
            if dcut is not None:
                dcut = _unsort_edges(dcut, csr)
        return drbf, dcut, dh, dw1, db1, dw2, db2, None, ddn, None, None


def cfconv(rbf, cut, h, csr, lin_a, lin_b, dist=None):
    """CFConv aggregation  out_i = sum_{e: j -> i} h_j * W(rbf_e) * cut_e  (W = lin_b(ssp(lin_a(.)))) as one autograd node
    differentiable in rbf [E, G], cut [E] and h (and the filter network's parameters): what a force evaluation needs.  The
    per-edge gradients come from ONE extra launch of csrc/cfconv_de.hip, in the caller's edge order and dtype, only for inputs
    that require them.  Callers check cfconv_edge_ok first (other shapes: the general composition of nn.CFConv.aggregate).
    dist = (d_norm [E] fp32, offsets [G] fp32, coeff): a promise that rbf = rbf_expand(d_norm) on these centres (detached).  The
    backward then hands d_norm its gradient from the kernel's fused distance epilogue; no [E, G] gradient is ever stored."""
    if not cfconv_edge_ok(rbf, h, lin_a.weight, lin_b.weight):
        raise MdlError("cfconv: unsupported shape F=%d G=%d %s (mdl_cfconv_bwd_edge_supported)" % (h.shape[1], rbf.shape[1], h.dtype))
    if rbf.shape[0] != csr.E:
        raise MdlError("cfconv: rbf must have one row per edge of the CSR")
    args = (cut, h, lin_a.weight, lin_a.bias, lin_b.weight, lin_b.bias, csr)
    if dist is None:
        return _CFConv.apply(rbf, *args, None, None, None)
    d_norm, offsets, coeff = _check_dist("cfconv", dist, rbf, "rbf")
    return _CFConv.apply(rbf.detach(), *args, d_norm, (offsets.float().contiguous(), float(coeff)), None)


def cfconv_dist_grad(h, edge_index, d_norm, cut, w1, b1, w2, b2, grad_out, csr=None, start=0.0, stop=1.0, resolution=50, width=0.2,
                     scale=1.0, edge_attr=None, out=None, want_dcut=False):
    """dL/dd of ONE CFConv aggregation whose edge features are rbf_expand(d_norm, start, stop, resolution, width) in h's dtype,
    for the output gradient grad_out [N, F]: the fused distance epilogue of csrc/cfconv_de.hip (the [E, G] gradient stays in
    registers).  cut [E]: the cutoff factors (constants here).  `scale` is the chain-rule factor of the caller's normalisation.
    Returns [E] fp32 in the caller's edge order — or (dd, dcut) with want_dcut, dcut [E] fp32 the gradient w.r.t. the cutoff
    factor; `out` ([E] fp32, CSR-ordered edge lists only) is added into instead, so that the blocks of a model accumulate in one
    buffer.  No atomics: bitwise repeatable.  No gradient flows through this call itself."""
    require_hip(h, d_norm, w1, w2, grad_out, cut)
    with torch.no_grad():
        F, G = h.shape[1], int(resolution)
        if not lib().mdl_cfconv_bwd_edge_supported(F, G, dtype_code(h)):
            raise MdlError("cfconv_dist_grad: unsupported F=%d G=%d" % (F, G))
        csr, offsets, d_sorted, ea = _dist_grad_inputs("cfconv_dist_grad", h, edge_index, d_norm, csr, start, stop, G, width, edge_attr, out)
        E = csr.E
        w1f, b1f, w2f, b2f = _f32c(w1), _f32c(b1), _f32c(w2), _f32c(b2)
        wpack = _cfconv_pack(w1f, b1f, w2f, b2f, F, G, h.device) if h.dtype == torch.bfloat16 else None
        dd = out if out is not None else torch.zeros(E, dtype=torch.float32, device=h.device)
        dcut = torch.zeros(E, dtype=torch.float32, device=h.device) if want_dcut else None
        _cfconv_bwd_edge_launch(ea, _sort_edges(cut.detach().float(), csr).contiguous(), h.detach().contiguous(),
                                grad_out.detach().to(h.dtype).contiguous(), csr, wpack, w1f, b1f, w2f, b2f, dcut=dcut, d_sorted=d_sorted,
                                offsets=offsets, coeff=rbf_coeff(start, stop, width), scale=scale, dd=dd)
        dd = dd if out is not None else _unsort_edges(dd, csr)
        return (dd, _unsort_edges(dcut, csr)) if want_dcut else dd


# ------------------------------------------------------------------------------------------------
# K7 — NNConv edge contraction  m_e = Y[src_e] (Co x D3) . h_e   (csrc/nnconv.hip)
# ------------------------------------------------------------------------------------------------
class _NNConvMsg(torch.autograd.Function):
    @staticmethod
    def forward(ctx, Y, h, csr, Co, D3):
        require_hip(Y, h)
        if Y.dtype != h.dtype:
            raise MdlError("nnconv_msg: Y (%s) and h (%s) must share a dtype" % (Y.dtype, h.dtype))
        Y, h = Y.contiguous(), h.contiguous()
        rowptr_s, _, eid_s, _ = csr.transposed()
        # padded static batch (HIP-graph replay): the unused edge slots belong to no by-source segment, so neither kernel
        # writes their rows — they must read as zeros (finite forward values, exactly zero gradients on every padded row)
        ctx.padded = _true_rows_for(h.shape[0]) is not None
        m = (torch.zeros if ctx.padded else torch.empty)((csr.E, Co), dtype=Y.dtype, device=Y.device)
        check(_launch_timed("nnconv_fwd", lambda: lib().mdl_nnconv_msg_fwd(
            ptr(Y), ptr(h), ptr(rowptr_s), ptr(eid_s), ptr(m), csr.N, Co, D3, dtype_code(Y), stream())), "mdl_nnconv_msg_fwd")
        ctx.csr, ctx.dims = csr, (Co, D3)
        ctx.save_for_backward(Y, h)
        return m

    @staticmethod
    def backward(ctx, dm):
        Y, h = ctx.saved_tensors
        Co, D3 = ctx.dims
        rowptr_s, _, eid_s, _ = ctx.csr.transposed()
        dm = dm.contiguous()
        dh, dY = (torch.zeros_like(h) if ctx.padded else torch.empty_like(h)), torch.empty_like(Y)
        check(lib().mdl_nnconv_msg_bwd(ptr(Y), ptr(h), ptr(dm), ptr(rowptr_s), ptr(eid_s), ptr(dh), ptr(dY), ctx.csr.N, Co,
                                       D3, dtype_code(Y), stream()), "mdl_nnconv_msg_bwd")
        return dY, dh, None, None, None


def nnconv_msg(Y, h, csr, out_channels):
    """m[e] = Y[src_e].view(Co, D3) @ h[e]  (caller's edge order): Y [N, Co*D3], h [E, D3] -> [E, Co]."""
    D3 = h.shape[1]
    if Y.shape[1] != out_channels * D3:
        raise MdlError("nnconv_msg: Y has %d columns, expected %d x %d" % (Y.shape[1], out_channels, D3))
    return _NNConvMsg.apply(Y, h, csr, int(out_channels), int(D3))


# ------------------------------------------------------------------------------------------------
# dense Linear on many rows (nodes / graphs): library GEMMs for the forward and dX, the tall-skinny TN HIP
# GEMM for the weight gradient — dW = g^T x contracts over the ROWS (2e5 nodes, 8192 graphs), a shape the
# library handles badly (47 us for a 64 x 64 x 8192 product, 0.7 ms for 64 x 114 x 2e5)
# ------------------------------------------------------------------------------------------------
_TN_COLSUM = True
_DENSE_BWD_WIDE = True   # ... also when both widths exceed 128 (SchNet's 150 x 150 filter layer)
_DENSE_BWD = True     # dX + dW + db of a tall dense layer in one pass (csrc/dense_bwd.hip)


# --- what the kernels admit, each window stated once: shapes alone (tests/test_dense_budget_host.py sweeps them), then operands ---
def _hip_shape_ok(M, K):
    """(out, in) features the streaming dense kernels take: linear.hip forward and gemm_tn.hip weight gradient."""
    return 1 <= M <= 160 and 4 <= K <= 256 and K % 2 == 0 and (M <= 128 or (K <= 160 and M % 2 == 0))


def _fused_fwd_shape_ok(M, K, act):
    """the fused forward GEMM + bias + activation (_LinearActTN) takes an [M, K] layer followed by `act`"""
    # (ssp: the one-pass softplus backward works on element PAIRS — an odd width would reach it with an odd element count)
    return act in ("relu", "ssp", None) and _hip_shape_ok(M, K) and (act != "ssp" or M % 2 == 0)


def _dense_bwd_shape_ok(M, K, has_bias, wide=True):
    """mdl_dense_bwd takes an [M, K] layer: even widths in [34, 160], the bias sums in column K; wide: also both sides above 128"""
    kb = K + (1 if has_bias else 0)
    return 34 <= min(M, K) and M <= 160 and kb <= 160 and M % 2 == 0 and K % 2 == 0 and (wide or not (M > 128 and kb > 128))


def _relu_bn_shape_ok(M, K, has_bias, tables=0):
    """_LinearReluBN: the one-pass backward's shapes (never both above 128), M % 4, at most three tables and M <= 128 with them"""
    return _dense_bwd_shape_ok(M, K, has_bias, wide=False) and M % 4 == 0 and tables <= 3 and (M <= 128 or not tables)


def _tn_colsum_shape_ok(M, K):
    """the streaming TN kernel forms column sums (db) / stages an activation: even widths, the ones column K inside the fifth tile"""
    return 1 <= M <= 160 and M % 2 == 0 and K % 2 == 0 and K <= 158


def _dword_rows(t):
    """rows of 2-byte elements the kernels address as dwords: unit column stride, even row stride, base on a dword"""
    return t.stride(1) == 1 and t.stride(0) % 2 == 0 and t.data_ptr() % 4 == 0


def _tn_split_ok(x, weight):
    """dW of a Linear with 256 < in <= 512 as two TN-GEMM halves (_tn_plan): even widths, dword-aligned halves"""
    M, K = weight.shape
    kh = (K // 2 + 1) & ~1
    return K <= 512 and K % 2 == 0 and M % 2 == 0 and M <= 128 and _dword_rows(x) and kh <= 256 and K - kh <= 256


def _tn_wide_out_ok(x, weight):
    """dW of a Linear with MANY outputs and few inputs (the GRU's 3C x C gate matrices, mpnn.py:160-161) as TN GEMMs of the
    TRANSPOSED product: dW^T[K, M] = x^T g in column chunks of <= 150 outputs (_tn_plan)"""
    M, K = weight.shape
    return 160 < M <= 600 and M % 2 == 0 and 4 <= K <= 160 and K % 2 == 0 and _dword_rows(x)


def _linear_tn_ok(x, weight):
    """the launches of _tn_plan form the weight gradient of this layer (ops.linear)"""
    M, K = weight.shape
    return (M <= 128 or _hip_shape_ok(M, K) or _tn_wide_out_ok(x, weight)) and (K <= 256 or _tn_split_ok(x, weight))


def _dx_hip_ok(g, w):
    M, K = w.shape
    return (g.dtype == torch.bfloat16 and g.is_cuda and g.shape[0] >= _DENSE_MIN_ROWS and g.is_contiguous() and g.data_ptr() % 16 == 0
            and _hip_shape_ok(K, M) and M % 2 == 0)


def _dense_bwd_ok(ctx, g, x, w, y=None):
    """mdl_dense_bwd takes this layer's backward: the input gradient is wanted, its shape window, dword-addressable bf16 rows."""
    return (_DENSE_BWD and ctx.needs_input_grad[0] and g.is_cuda and g.shape[0] >= _DENSE_MIN_ROWS and w.is_contiguous()
            and _dense_bwd_shape_ok(*ctx.shape, ctx.has_bias, _DENSE_BWD_WIDE) and g.dtype == x.dtype == w.dtype == torch.bfloat16
            and _dword_rows(g) and _dword_rows(x) and (y is None or (y.dtype == torch.bfloat16 and _dword_rows(y))))


def _tn_act_ok(ctx, g, x, y, w=None):
    """The activation derivative can go into the staging of the backward products instead of a pass of its own: the TN
    GEMM (dW, db) always, the dX product when it runs on the streaming kernel (or is not wanted)."""
    M, K = ctx.shape
    if ctx.needs_input_grad[0] and not (w is not None and g.is_contiguous() and y.is_contiguous() and _dx_hip_ok(g, w)):
        return False
    return (_TN_COLSUM and _hip_shape_ok(M, K) and _tn_colsum_shape_ok(M, K) and g.dtype == torch.bfloat16
            and _dword_rows(g) and _dword_rows(x) and _dword_rows(y))


def _lowp_pair(lowp, x):
    """the step's low-precision copies (weight, bias) of a layer if they are in x.dtype, else (None, None)"""
    return lowp if lowp is not None and lowp[0].dtype == x.dtype else (None, None)


def _wb(x, weight, bias, w_lp=None, b_lp=None):
    """(w, b) in x.dtype from the fp32 masters, or the caller's copies w_lp / b_lp already in x.dtype (one multi-tensor cast per
    step instead of two launches per layer).  Called inside a node's forward: no autograd, the gradients go to the masters."""
    b = None if bias is None else (bias.to(x.dtype) if b_lp is None else b_lp)
    return (weight.to(x.dtype) if w_lp is None else w_lp), b


def _dw_db_zeros(M, K, device, db=True):
    """fp32 zeros for dW (flat, M * K) | db [M] out of the step's gradient arena (one fill per step)"""
    buf = _zeros_grad(M * K + (M if db else 0), device)
    return buf[:M * K], buf[M * K:]


def _table_args(idx, tables):
    """K6's three (table, index) pointer slots, and the dense tables behind them (to be held until the launch is enqueued)"""
    tabs = [None if t is None else t.contiguous() for t in tables] + [None] * (3 - len(tables))
    return [ptr(v) for slot in zip(tabs, list(idx) + [None] * (3 - len(idx))) for v in slot], tabs


def _table_grads(g, idx, rows, needs):
    """the gathered tables' gradients: segment sums of the layer's gradient rows g (needs is never set for an absent table)"""
    return tuple(scatter(g, ix, 0, r, "sum") if need else None for ix, r, need in zip(idx, rows, needs))


def _dx_hip(g, w, act_y=None):
    """dX = g W for a tall bf16 g through the streaming dense kernel (the 'weight' of that product is W^T): the library
    picks a 64x64x256 macro tile for [1.5e6, 150] x [150, 150] and runs it at 35 TFLOP/s (1.9 ms); as a stream it is
    E*(M+K)*2 bytes.  act_y = (code, y): g is the gradient w.r.t. the activated output y; the activation derivative is
    applied while the kernel stages its input (mdl_linear_act_in) — callers check _dx_hip_ok first."""
    M, K = w.shape
    if _dx_hip_ok(g, w):
        wt = w.t().contiguous()
        dx = torch.empty((g.shape[0], K), dtype=g.dtype, device=g.device)
        if act_y is not None:
            check(lib().mdl_linear_act_in(ptr(g), ptr(act_y[1]), act_y[0], ptr(wt), None, ptr(dx), g.shape[0], M, K, 0,
                                          dtype_code(g), stream()), "mdl_linear_act_in(dX)")
        else:
            check(lib().mdl_linear_act(ptr(g), ptr(wt), None, ptr(dx), g.shape[0], M, K, 0, dtype_code(g), stream()),
                  "mdl_linear_act(dX)")
        return dx
    assert act_y is None
    return g @ w


def _dense_bwd(ctx, g, x, w, act_y=None, xout=0, want_gm=False):
    """(dx, dW, db[, g']) of y = act(x W^T + b) from ONE pass over g, y, x (callers check _dense_bwd_ok); act_y = (code, y):
    g is the gradient w.r.t. the activated output; xout: x is the relu (1) / shifted-softplus (2) output of a private layer in
    front and dx is returned w.r.t. that layer's pre-activation; want_gm: also return g' = g .* act'(y) (bf16, dense)."""
    M, K = ctx.shape
    N = g.shape[0]
    dw, dbv = _dw_db_zeros(M, K, g.device)
    dx = torch.empty((N, K), dtype=g.dtype, device=g.device)
    gm = torch.empty((N, M), dtype=g.dtype, device=g.device) if want_gm else None
    code, y = act_y if act_y is not None else (0, None)
    check(lib().mdl_dense_bwd_ex(ptr(g), g.stride(0), M, ptr(y), 0 if y is None else y.stride(0), code, ptr(x), x.stride(0), K,
                                 ptr(w), ptr(dx), K, xout, ptr(gm), ptr(dw), ptr(dbv) if ctx.has_bias else None,
                                 ptr(_tn_scratch(g.device, N)), N, dtype_code(g) | _dflag(), stream()), "mdl_dense_bwd")
    out = (dx, dw.view(M, K).to(ctx.wdtype), dbv.to(ctx.wdtype) if ctx.has_bias else None)
    return out + (gm,) if want_gm else out


def _tn_plan(M, K, has_bias, ldg, ldx):
    """The TN-GEMM launches that form dW (and db) of an [M, K] layer from g [N, M] (row stride ldg; an odd M is padded first) and
    x [N, K] (row stride ldx), one (kernel M, kernel K, lda, ldb, column sums, lo, hi) per launch:
      M > 160   many outputs, few inputs: dW^T = x^T g[:, lo:hi], one launch per chunk of <= 150 gradient columns (the library
                runs the (M x N)(N x K) form of this N ~ 6e4 contraction at 234 us for 300 x 100; this is 2 x ~15 us)
      K > 256   wide inputs (MEGNet's node block: [x | v_e | u[batch]] = 3d columns): the kernel takes <= 256 input columns, so
                two products over the column halves x[:, lo:hi] (the library: 335 us for 100 x 300 x 1e5, on 9 workgroups)
      else      one launch over x[:, 0:K]
    column sums: db out of the same pass (the sums of g ride in a padding column of the B tile and are flushed with one gathered
    atomic instruction per block) where the layer has a bias and the kernel-level shape allows; else the library's reduction."""
    if M > 160:
        nch = -(-M // 150)
        mc = ((M + nch - 1) // nch + 1) & ~1
        return [(K, min(m0 + mc, M) - m0, ldx, ldg, False, m0, min(m0 + mc, M)) for m0 in range(0, M, mc)]
    if K > 256:
        kh = (K // 2 + 1) & ~1
        return [(M, kh, ldg, ldx, has_bias and _tn_colsum_shape_ok(M, kh), 0, kh), (M, K - kh, ldg, ldx, False, kh, K)]
    return [(M, K, ldg, ldx, has_bias and _tn_colsum_shape_ok(M, K), 0, K)]


def _tn_dw_db(ctx, g, x, act_y=None):
    """(dW, db) of y = x W^T + b in the masters' dtype from the launches of _tn_plan, accumulated in fp32.  act_y = (code, y):
    g is the gradient w.r.t. the ACTIVATED output y and the derivative is applied inside the TN GEMM's staging (callers check
    _tn_act_ok).  db out of the same pass needs dword-addressable operands too; ops.configure(tn_colsum=False) turns it off."""
    M, K = ctx.shape
    code, y = act_y if act_y is not None else (0, None)
    # the streaming kernel stages rows as dwords: pad an odd width (the model's 1-column output layer) with a zero column
    ga = torch.nn.functional.pad(g, (0, 1)) if M % 2 else g
    Ma = ga.shape[1]
    plan = _tn_plan(Ma, K, ctx.has_bias, ga.stride(0), x.stride(0))
    fused_db = plan[0][4] and _TN_COLSUM and _dword_rows(ga) and _dword_rows(x)
    transposed = Ma > 160
    flat, dbv = _dw_db_zeros(Ma, K, g.device, db=not transposed)
    parts, off = [], 0
    for Mk, Kk, lda, ldb, colsum, lo, hi in plan:
        parts.append(flat[off:off + Mk * Kk].view(Mk, Kk))
        off += Mk * Kk
        a, b = (x, ga[:, lo:hi]) if transposed else (ga, x[:, lo:hi] if lo else x)              # (lo = 0: the same base address)
        check(_gemm_tn(a, lda, Mk, y, 0 if y is None else y.stride(0), code, b, ldb, Kk, parts[-1], dbv if colsum and fused_db else None,
                       g.shape[0], dtype_code(g) | _dflag(), g.device), "mdl_gemm_tn_act" if code else "mdl_gemm_tn_colsum")
    dw = parts[0] if len(parts) == 1 else torch.cat(parts, dim=1)
    dw = dw.t() if transposed else dw[:M]
    db = (dbv[:M] if fused_db else g.sum(dim=0, dtype=torch.float32)).to(ctx.wdtype) if ctx.has_bias else None
    return dw.to(ctx.wdtype), db


def _linear_tn_grads(ctx, g, x, w, act_y=None):
    """(dx, dW, db) of y = x W^T + b for a tall x: streaming HIP product (or library GEMM) for dx, _tn_dw_db for dW and db.
    act_y = (code, y): both apply the derivative of the ACTIVATED output y in their staging (_tn_act_ok), the TN GEMM first."""
    staged = _tn_dw_db(ctx, g, x, act_y) if act_y is not None else None
    dx = _dx_hip(g, w, act_y) if ctx.needs_input_grad[0] else None
    return (dx,) + (staged or _tn_dw_db(ctx, g, x))


def _linear_backward(ctx, g, x, w, code, out, in_act, want_masked_rows, stage_act=True):
    """(dx, dW, db, rows) of out = act(x W^T + b) for every dense node: THE place where the backward's route is chosen.
    code: the activation whose derivative g still lacks (0: none, or g already is w.r.t. the pre-activation), out: the saved
    activated output; in_act: x is the relu (1) / ssp (2) output of a private layer in front and dx is returned w.r.t. that
    layer's pre-activation (nn._seq's hand-over); want_masked_rows: also return rows = g .* act'(out), dense (K6's tables).
      1. one pass over g, out, x for everything, the hand-over in its epilogue (_dense_bwd_ok)
      2. the derivative in the staging of the TN GEMM and of the streaming dX (_tn_act_ok; stage_act=False: K6 never took it)
      3. the masked gradient materialised (library mask / mdl_ssp_bwd), then _linear_tn_grads; behind 2. and 3. the hand-over"""
    act_y = (code, out) if code else None
    if _dense_bwd_ok(ctx, g, x, w, out if code else None):
        res = _dense_bwd(ctx, g, x, w, act_y, xout=in_act, want_gm=bool(want_masked_rows and code))
        return res if len(res) > 3 else res + (g.contiguous() if want_masked_rows else None,)
    if code and stage_act and not want_masked_rows and _tn_act_ok(ctx, g, x, out, w):
        dx, dw, db = _linear_tn_grads(ctx, g, x, w, act_y)
    else:
        if code == 1:
            g = torch.ops.aten.threshold_backward(g, out, 0)
        elif code == 2:                            # d/dv (softplus(v) - ln2) = sigmoid(v) = 1 - exp(-(out + ln2))
            g = g.contiguous()
            dpre = torch.empty_like(g)
            check(lib().mdl_ssp_bwd(ptr(g), ptr(out), ptr(dpre), g.numel(), dtype_code(g), stream()), "mdl_ssp_bwd")
            g = dpre
        g = g.contiguous()
        dx, dw, db = _linear_tn_grads(ctx, g, x, w)
    if dx is not None and in_act:                  # the hand-over on the paths without the fused epilogue
        dx = (torch.ops.aten.threshold_backward(dx, x, 0) if in_act == 1 else
              (dx.float() * (1.0 - torch.exp(-(x.float() + _LN2)))).to(dx.dtype))
    return dx, dw, db, (g if want_masked_rows else None)


class _LinearTN(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, w_lp=None, b_lp=None):
        w, b = _wb(x, weight, bias, w_lp, b_lp)
        out = torch.nn.functional.linear(x, w, b)
        ctx.save_for_backward(x, w)
        ctx.wdtype, ctx.has_bias, ctx.shape = weight.dtype, bias is not None, tuple(weight.shape)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        return _linear_backward(ctx, g, x, w, 0, None, 0, False)[:3] + (None, None)


_MLP_HEAD = True        # post-FC head (post_lin_list + lin_out) as one launch per direction
_LINEAR_WIDE = True   # NNConv's Y = x W2r on the streaming kernel


class _LinearActTN(torch.autograd.Function):
    """act(x W^T + b) with the forward as ONE streaming HIP kernel (GEMM + bias + activation) and the backward of
    _LinearTN (one-pass dense backward, or library dX + TN GEMM for dW and db); the ReLU mask comes from the saved output.

    Chains of such layers whose intermediate outputs nobody else sees (nn._seq) hand the activation derivative DOWN the chain:
    in_act = code of the activation that produced x (x is that layer's output): the input gradient is returned w.r.t. that
    layer's PRE-activation (dx .* act'(x), from the x tile the backward stages anyway); out_pre: the gradient arriving here
    already is w.r.t. this layer's pre-activation (the layer behind applied in_act), so no derivative, no read of the output."""

    @staticmethod
    def forward(ctx, x, weight, bias, w_lp, b_lp, act, in_act=0, out_pre=False, pre=None):
        # pre: this layer's output, already formed by a fused forward (cfconv_fused) — the node then only records the graph
        w, b = _wb(x, weight, bias, w_lp, b_lp)
        N, K = x.shape
        M = weight.shape[0]
        if pre is not None:
            out = pre.view_as(pre)
        else:
            out = torch.empty((N, M), dtype=x.dtype, device=x.device)
            check(lib().mdl_linear_act(ptr(x), ptr(w), ptr(b), ptr(out), N, K, M, _ACT_CODE.get(act, 0), dtype_code(x),
                                       stream()), "mdl_linear_act")
        ctx.save_for_backward(x, w, out if act in ("relu", "ssp") and not out_pre else None)
        ctx.wdtype, ctx.has_bias, ctx.shape, ctx.act = weight.dtype, bias is not None, tuple(weight.shape), act
        ctx.in_act, ctx.out_pre = int(in_act), bool(out_pre)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, out = ctx.saved_tensors
        code = 0 if ctx.out_pre else _ACT_CODE.get(ctx.act, 0)
        return _linear_backward(ctx, g, x, w, code, out, ctx.in_act, False)[:3] + (None,) * 6


class _LinearGatherAct(torch.autograd.Function):
    """K6: act(x W^T + bias + sum_i p_i[idx_i]) in one streaming HIP kernel; backward = masked gradient -> library dX,
    TN GEMM for dW (+ db), segmented sums of the gradient rows for the gathered tables."""

    @staticmethod
    def forward(ctx, x, weight, bias, act, idx, *tables):
        w, b = _wb(x, weight, bias)
        N, K = x.shape
        M = weight.shape[0]
        targs, tabs = _table_args(idx, tables)
        out = torch.empty((N, M), dtype=x.dtype, device=x.device)
        check(_launch_timed("edge_linear", lambda: lib().mdl_linear_gather_act(
            ptr(x), ptr(w), ptr(b), *targs, ptr(out), N, K, M, 1 if act == "relu" else 0, dtype_code(x), stream())),
            "mdl_linear_gather_act")
        ctx.save_for_backward(x, w, out if act == "relu" else None)
        ctx.idx, ctx.rows = list(idx), [None if t is None else t.shape[0] for t in tabs]
        ctx.wdtype, ctx.has_bias, ctx.shape, ctx.act = weight.dtype, bias is not None, tuple(weight.shape), act
        return out

    @staticmethod
    def backward(ctx, g):
        x, w, out = ctx.saved_tensors
        needs = ctx.needs_input_grad[5:]
        dx, dw, db, rows = _linear_backward(ctx, g, x, w, 1 if ctx.act == "relu" else 0, out, 0, any(needs), stage_act=False)
        return (dx, dw, db, None, None) + _table_grads(rows, ctx.idx, ctx.rows, needs)


def linear_gather_act(x, weight, bias, act, gathered):
    """act(x W^T + bias + sum_i table_i[index_i]) for bf16 rows; `gathered` = [(table [rows, M], index [N] int), ...] (<= 3)."""
    ok = (act in ("relu", None) and x.dtype == torch.bfloat16 and x.is_cuda and x.dim() == 2 and x.is_contiguous()
          and weight.shape[0] <= 128 and 4 <= weight.shape[1] <= 256 and weight.shape[1] % 2 == 0 and x.data_ptr() % 16 == 0
          and len(gathered) <= 3 and x.shape[0] > 0)
    if not ok:
        y = linear(x, weight, bias)
        for tab, ix in gathered:
            y = y + gather(tab, ix)
        return y if act is None else getattr(torch.nn.functional, act)(y)
    idx = [ix if ix.dtype == torch.int32 else ix.to(torch.int32) for _, ix in gathered]
    return _LinearGatherAct.apply(x, weight, bias, act, idx, *[t.to(x.dtype) for t, _ in gathered])


def _ptr_array(tensors):
    import ctypes
    return (ctypes.c_void_p * len(tensors))(*[None if t is None else t.data_ptr() for t in tensors])


class _MlpHead(torch.autograd.Function):
    """relu(...relu(x W_0^T + b_0)...) W_last^T + b_last as one launch forward and one backward (csrc/mlp.hip): the post-FC
    head on the pooled graph rows.  params = (W_0, b_0, ..., W_last, b_last) fp32 masters; lowp = their bf16 copies or None."""

    @staticmethod
    def forward(ctx, x, lowp, f32_out, *params):
        import ctypes
        NL = len(params) // 2
        wb = [_wb(x, params[2 * l], params[2 * l + 1], *((None, None) if lowp is None or lowp[l] is None else lowp[l]))
              for l in range(NL)]
        ws, bs = [w.contiguous() for w, _ in wb], [b for _, b in wb]
        N, K0 = x.shape
        M = [int(w.shape[0]) for w in ws]
        # f32_out: the prediction as fp32 rows (the values the bf16 output holds) — the model's `out.float()` behind the head and
        # the cast of the loss gradient in front of its backward are then no launches (MDL_MLP_F32_IO)
        hs = [torch.empty((N, m), dtype=torch.float32 if (f32_out and l == NL - 1) else x.dtype, device=x.device)
              for l, m in enumerate(M)]
        Ma = (ctypes.c_int * NL)(*M)
        io = _lib.MDL_MLP_F32_IO if f32_out else 0
        check(lib().mdl_mlp_head_fwd(ptr(x), _ptr_array(ws), _ptr_array(bs), _ptr_array(hs), N, K0, NL, Ma, dtype_code(x) | io,
                                     stream()), "mdl_mlp_head_fwd")
        ctx.save_for_backward(x, *ws, *hs[:-1])
        ctx.NL, ctx.M, ctx.K0, ctx.io = NL, M, K0, io
        ctx.has_bias = [params[2 * l + 1] is not None for l in range(NL)]
        ctx.wdtypes = [params[2 * l].dtype for l in range(NL)]
        return hs[-1]

    @staticmethod
    def backward(ctx, gy):
        import ctypes
        saved = ctx.saved_tensors
        NL, M, K0 = ctx.NL, ctx.M, ctx.K0
        x, ws, hs = saved[0], list(saved[1:1 + NL]), list(saved[1 + NL:])
        N = x.shape[0]
        gy = gy.contiguous()
        if gy.dtype != (torch.float32 if ctx.io else x.dtype):
            gy = gy.to(torch.float32 if ctx.io else x.dtype)
        Ks = [K0] + M[:-1]
        dws, dbs = [], []
        for l in range(NL):
            flat, dbv = _dw_db_zeros(M[l], Ks[l], x.device)
            dws.append(flat.view(M[l], Ks[l]))
            dbs.append(dbv if ctx.has_bias[l] else None)
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        Ma = (ctypes.c_int * NL)(*M)
        check(lib().mdl_mlp_head_bwd(ptr(x), _ptr_array(ws), _ptr_array(hs + [None]), ptr(gy), ptr(dx), _ptr_array(dws), _ptr_array(dbs),
                                     N, K0, NL, Ma, dtype_code(x) | _dflag() | ctx.io, stream()), "mdl_mlp_head_bwd")
        grads = []
        for l in range(NL):
            grads.append(dws[l].to(ctx.wdtypes[l]))
            grads.append(dbs[l].to(ctx.wdtypes[l]) if ctx.has_bias[l] else None)
        return (dx, None, None) + tuple(grads)


def mlp_head_ok(x, lins, act):
    """the fused head takes bf16 rows on the device, 1..4 dense layers of width <= 64 (hidden widths even) with ReLU between.
    Any row count: at the reference's batch size (100 graphs, config.yml:136) the layer-by-layer fallback is ~35 launches of
    4-8 us each (library GEMMs, casts, ReLU masks, bias sums) against two."""
    if not (_MLP_HEAD and act == "relu" and x.dtype == torch.bfloat16 and x.is_cuda and x.dim() == 2 and x.is_contiguous()
            and 1 <= len(lins) <= 4 and x.shape[0] >= 1 and 2 <= x.shape[1] <= 64 and x.shape[1] % 2 == 0 and x.data_ptr() % 4 == 0):
        return False
    k = x.shape[1]
    for j, lin in enumerate(lins):
        if lin.in_features != k or not 1 <= lin.out_features <= 64 or (j + 1 < len(lins) and lin.out_features % 2) or not lin.weight.requires_grad:
            return False
        k = lin.out_features
    return True


def mlp_head(x, lins, lowp=None, f32_out=False):
    """lins: the nn.Linear modules of the chain (ReLU after every one but the last); f32_out: the last layer's output as fp32 rows
    (the bf16-rounded values; for a head whose output is the model's fp32 prediction)"""
    params = []
    for lin in lins:
        params += [lin.weight, lin.bias]
    return _MlpHead.apply(x, lowp, bool(f32_out), *params)


class _LinearWide(torch.autograd.Function):
    """y = x @ w for a wide w [K, M] (M in the thousands): forward as a streaming HIP kernel over 192-column blocks
    (mdl_linear_wide), backward = the two library products autograd would form."""

    @staticmethod
    def forward(ctx, x, w):
        N, K = x.shape
        M = w.shape[1]
        wt = w.t().contiguous()                                        # [M, K] rows for the kernel (2 MB for NNConv's W2r)
        out = torch.empty((N, M), dtype=x.dtype, device=x.device)
        check(lib().mdl_linear_wide(ptr(x), ptr(wt), ptr(out), N, K, M, dtype_code(x), stream()), "mdl_linear_wide")
        ctx.save_for_backward(x, w)
        return out

    @staticmethod
    def backward(ctx, g):
        x, w = ctx.saved_tensors
        dx = g @ w.t() if ctx.needs_input_grad[0] else None
        dw = x.t() @ g if ctx.needs_input_grad[1] else None
        return dx, dw


def matmul_wide(x, w):
    """x @ w; bf16 tall x (even K <= 160) with a wide w take the streaming kernel for the forward product."""
    if (_LINEAR_WIDE and x.dtype == torch.bfloat16 and w.dtype == torch.bfloat16 and x.is_cuda and x.dim() == 2 and x.is_contiguous()
            and x.shape[0] >= 1024 and x.shape[1] % 2 == 0 and 4 <= x.shape[1] <= 160 and w.shape[1] >= 640
            and x.data_ptr() % 16 == 0):
        return _LinearWide.apply(x, w)
    return x @ w


def linear_act_fused_ok(x, weight, act):
    """the fused dense layer (_LinearActTN) takes (x, weight, act)"""
    return (x.dtype == torch.bfloat16 and x.is_cuda and x.dim() == 2 and x.is_contiguous() and x.shape[0] >= _DENSE_MIN_ROWS
            and _fused_fwd_shape_ok(weight.shape[0], weight.shape[1], act) and x.data_ptr() % 16 == 0 and weight.requires_grad)


def linear_act(x, weight, bias, act, lowp=None, in_act=None, out_pre=False, pre=None):
    """getattr(F, act)(F.linear(x, weight, bias)) — fused forward for bf16 inputs with dense rows, even in <= 256,
    out <= 128 and act in (relu, ssp, none); anything else composes `linear` with the library activation.
    in_act / out_pre: the activation hand-over of a private chain (see _LinearActTN; callers check linear_act_fused_ok for
    both layers first)."""
    if linear_act_fused_ok(x, weight, act):
        return _LinearActTN.apply(x, weight, bias, *_lowp_pair(lowp, x), act, _ACT_CODE.get(in_act, 0), out_pre, pre)
    assert not in_act and not out_pre and pre is None, "linear_act: activation hand-over on a layer that is not fused"
    y = linear(x, weight, bias, lowp)
    if act is None:
        return y
    if act == "ssp":
        return torch.nn.functional.softplus(y) - _LN2
    return getattr(torch.nn.functional, act)(y)


# ------------------------------------------------------------------------------------------------
# First-edge-layer distance gradient (csrc/linear_de.hip): forces for MEGNet and MPNN.  In both models the positions enter
# through a Linear(G -> M) + ReLU applied to edge_attr = rbf_expand(d_norm); the layer's input gradient collapses through the
# expansion to one number per edge inside the kernel, and no [E, G] gradient is stored.
# ------------------------------------------------------------------------------------------------
# launches of mdl_linear_rbf_dist_grad (tests assert that the kernel, not the general composition, served a case)
LIN_DD_LAUNCHES = collections.Counter()


def linear_dist_ok(y, weight):
    """mdl_linear_rbf_dist_grad takes the gradient of this layer output: [E, M] fp32 / bf16 rows on a HIP device, M <= 256, G <= 64"""
    if not (y.is_cuda and y.dim() == 2 and weight.dim() == 2 and y.shape[1] == weight.shape[0]
            and y.dtype in (torch.float32, torch.bfloat16)):
        return False
    return bool(lib().mdl_linear_rbf_dist_grad_supported(weight.shape[0], weight.shape[1], dtype_code(y)))


def _rows(t):
    """t [E, M] with unit column stride and a leading dimension >= M (what autograd hands a backward may be an expanded view)"""
    return t if t.stride(1) == 1 and (t.shape[0] <= 1 or t.stride(0) >= t.shape[1]) else t.contiguous()


def _linear_dd_launch(g, act_y, w, d_norm, offsets, coeff, scale, dd, accumulate):
    """mdl_linear_rbf_dist_grad: dd [E] fp32 = or += the distance gradient of the layer with weight w [M, G] (g's dtype)"""
    LIN_DD_LAUNCHES["distance"] += 1
    E, M = g.shape
    g = _rows(g)
    act_y = None if act_y is None else _rows(act_y)
    check(_launch_timed("linear_dd", lambda: lib().mdl_linear_rbf_dist_grad(
        ptr(g), g.stride(0) if E > 1 else M, ptr(act_y), M if act_y is None or E <= 1 else act_y.stride(0), ptr(w), dtype_code(g),
        ptr(d_norm), ptr(offsets), float(coeff), float(scale), ptr(dd), int(bool(accumulate)), E, M, w.shape[1], stream())),
        "mdl_linear_rbf_dist_grad")


class _LinearDist(torch.autograd.Function):
    """The node BEHIND a dense layer y = act(W rbf_expand(d_norm) + b) that closes the chain to the distance.  Forward: y itself,
    handed through (the layer's own node made it, bit for bit as ever, and keeps forming dW / db).  Backward: the arriving
    gradient goes on to the layer's node unchanged, and d_norm receives dL/dd_norm from mdl_linear_rbf_dist_grad.
    masked: g is the gradient w.r.t. the ReLU output y (the mask is applied in the kernel); otherwise w.r.t. the
    pre-activation — the chain behind the layer applied the derivative (nn._seq's hand-over) or there is no activation."""

    @staticmethod
    def forward(ctx, y, w, d_norm, offsets, coeff, masked):
        ctx.save_for_backward(y if masked else None, w, d_norm, offsets)
        ctx.coeff = coeff
        return y.view_as(y)

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        y, w, d_norm, offsets = ctx.saved_tensors
        dd = None
        if ctx.needs_input_grad[2]:
            dd = torch.empty(d_norm.numel(), dtype=torch.float32, device=g.device)
            _linear_dd_launch(g, y, w, d_norm, offsets, ctx.coeff, 1.0, dd, False)
        return g, None, dd, None, None, None


def expansion_of(dist, dtype):
    """rbf_expand of dist = (d_norm, offsets, coeff) as a tensor that carries the gradient to d_norm: the general composition"""
    return _RbfExpand.apply(dist[0].contiguous(), dist[1].float().contiguous(), float(dist[2]), dtype)


def rbf_linear_act(edge_attr, weight, bias, act, dist, lowp=None, out_pre=False, fused=True, layer=None):
    """act(F.linear(edge_attr, weight, bias)) for edge_attr = rbf_expand(d_norm), differentiable in d_norm.
    dist = (d_norm [E] fp32, offsets [G] fp32, coeff): a promise that edge_attr is the Gaussian expansion of d_norm on these
    centres (as ops.cgconv / ops.cfconv take it).  The forward is bit for bit the layer's usual one from the given edge_attr —
    the library product + activation for equal dtypes (`layer`: the module to call for it, e.g. a SplitLinear), ops.linear_act
    with `lowp` / `out_pre` for bf16 rows (nn._seq's hand-over included) — and the weight and bias gradients come from the same
    nodes as ever.  When d_norm requires a gradient, one more node behind the layer returns dL/dd_norm from
    csrc/linear_de.hip; edge_attr is detached and no [E, G] gradient exists.  Other activations than relu / None, shapes the
    kernel does not take (M > 256, G > 64) and fused=False use the general composition: the expansion carries the gradient,
    then the dense layer's input gradient and mdl_rbf_expand_bwd."""
    d_norm, offsets, coeff = _check_dist("rbf_linear_act", dist, edge_attr, "edge_attr")
    want = torch.is_grad_enabled() and d_norm.requires_grad
    ok = want and fused and act in ("relu", None) and edge_attr.dim() == 2 and tuple(weight.shape[1:]) == (edge_attr.shape[1],)
    ok = ok and bool(lib().mdl_linear_rbf_dist_grad_supported(weight.shape[0], weight.shape[1], dtype_code(edge_attr)))
    if ok:
        edge_attr = edge_attr.detach()
    elif want:
        edge_attr = expansion_of(dist, edge_attr.dtype)
    if edge_attr.dtype == weight.dtype:
        y = layer(edge_attr) if layer is not None else torch.nn.functional.linear(edge_attr, weight, bias)
        if act == "ssp":
            y = torch.nn.functional.softplus(y) - _LN2
        elif act is not None:
            y = getattr(torch.nn.functional, act)(y)
    else:
        y = linear_act(edge_attr, weight, bias, act, lowp, None, out_pre, None)
    if not ok:
        return y
    w = _wb(y, weight.detach(), None, _lowp_pair(lowp, y)[0])[0].detach()
    return _LinearDist.apply(y, w.contiguous(), d_norm, offsets.float().contiguous(), float(coeff), act == "relu" and not out_pre)


def linear_dist_grad(g, weight, d_norm, act_y=None, start=0.0, stop=1.0, resolution=50, width=0.2, scale=1.0, out=None):
    """dL/dd of ONE dense layer y = act(W rbf_expand(d_norm, start, stop, resolution, width) + b) for the gradient g [E, M]:
    w.r.t. the layer's pre-activation (act_y None), or w.r.t. its ReLU output act_y [E, M] (the mask is applied in the kernel).
    weight [M, resolution] is used in g's dtype (fp32, or the bf16 copy the forward multiplies); g and act_y may be column
    slices of wider tensors.  `scale` is the chain-rule factor of the caller's normalisation.  Returns [E] fp32; `out` ([E]
    fp32) is added into instead, so that the layers of a model accumulate in one buffer.  Purely per edge: any edge order, no
    atomics, bitwise repeatable.  No gradient flows through this call itself."""
    require_hip(g, weight, d_norm)
    with torch.no_grad():
        G = int(resolution)
        if g.dim() != 2 or tuple(weight.shape) != (g.shape[1], G) or not linear_dist_ok(g, weight):
            raise MdlError("linear_dist_grad: unsupported g %s / weight %s %s (mdl_linear_rbf_dist_grad_supported)"
                           % (tuple(g.shape), tuple(weight.shape), g.dtype))
        E = g.shape[0]
        if d_norm.dtype != torch.float32 or d_norm.numel() != E:
            raise MdlError("linear_dist_grad: d_norm must be [E] float32 over the %d rows of g" % E)
        if act_y is not None and (act_y.shape != g.shape or act_y.dtype != g.dtype):
            raise MdlError("linear_dist_grad: act_y must have g's shape and dtype")
        if out is not None and (out.dtype != torch.float32 or out.numel() != E or not out.is_contiguous()):
            raise MdlError("linear_dist_grad: out must be a contiguous [E] float32 tensor")
        offsets = rbf_offsets(start, stop, G, g.device)
        dd = out if out is not None else torch.empty(E, dtype=torch.float32, device=g.device)
        _linear_dd_launch(g.detach(), None if act_y is None else act_y.detach(), weight.detach().to(g.dtype).contiguous(),
                          d_norm.detach().contiguous(), offsets, rbf_coeff(start, stop, width), scale, dd, out is not None)
        return dd


class _LinearSplitTN(torch.autograd.Function):
    """F.linear on fp32 tensors whose WEIGHT GRADIENT dW = g^T x (contraction over the rows: N ~ 2e5 for a node-level layer) runs
    as three bf16 TN-GEMM launches on (hi, lo)-split operands (mdl_split_bf16 + mdl_gemm_tn, fp32 accumulation) instead of the
    library's fp32 product (0.6 ms for the pre-FC layer of the bench batch against 3 x 0.03): the "bf16x3" parity mode.  Forward
    and dX stay the library's exact fp32 products."""

    @staticmethod
    def forward(ctx, x, weight, bias):
        ctx.save_for_backward(x, weight)
        ctx.has_bias = bias is not None
        return torch.nn.functional.linear(x, weight, bias)

    @staticmethod
    def backward(ctx, g):
        x, weight = ctx.saved_tensors
        g = g.contiguous()
        M, K = weight.shape
        N = x.shape[0]
        dx = g @ weight if ctx.needs_input_grad[0] else None

        def split(t):
            t = t.contiguous()
            hi, lo = torch.empty_like(t, dtype=torch.bfloat16), torch.empty_like(t, dtype=torch.bfloat16)
            check(lib().mdl_split_bf16(ptr(t), ptr(hi), ptr(lo), t.numel(), stream()), "mdl_split_bf16")
            return hi, lo
        xh, xl = split(x)
        gh, gl = split(g)
        dw = torch.zeros((M, K), dtype=torch.float32, device=x.device)
        fl = _dflag()
        for a, b in ((gl, xh), (gh, xl), (gh, xh)):
            check(_gemm_tn(a, M, M, None, 0, 0, b, K, K, dw, None, N, _lib.MDL_BF16 | fl, x.device), "mdl_gemm_tn")
        db = g.sum(0) if ctx.has_bias else None
        return dx, dw.to(weight.dtype), db


def linear_split_ok(x, weight):
    """shapes of _LinearSplitTN: fp32 rows on a HIP device, enough of them, even widths inside mdl_gemm_tn's limits"""
    M, K = weight.shape
    return (x.is_cuda and x.dtype == torch.float32 and weight.dtype == torch.float32 and x.dim() == 2 and x.shape[0] >= 1024
            and M % 2 == 0 and K % 2 == 0 and ((M <= 128 and K <= 256) or (M <= 160 and K <= 160))
            and weight.requires_grad and torch.is_grad_enabled() and not _DET)


def linear(x, weight, bias, lowp=None):
    """F.linear in the dtype of x (fp32 master weights); bf16 inputs with many rows, out <= 128, in <= 256 take the
    HIP TN GEMM for dW, anything else the library autograd path.  `lowp` = (weight, bias) already cast to x.dtype."""
    if (x.dtype == torch.bfloat16 and x.is_cuda and x.dim() == 2 and x.stride(1) == 1 and x.shape[0] >= _DENSE_MIN_ROWS
            and _linear_tn_ok(x, weight) and weight.requires_grad):
        return _LinearTN.apply(x, weight, bias, *_lowp_pair(lowp, x))
    return torch.nn.functional.linear(x, weight.to(x.dtype), None if bias is None else bias.to(x.dtype))


# ------------------------------------------------------------------------------------------------
# GRU gates (MPNN): one launch per direction instead of ~12 + ~25 elementwise / chunk / cat / cast launches
# ------------------------------------------------------------------------------------------------
class _GRUGates(torch.autograd.Function):
    """(h_new fp32, out) from gi, gh [N, 3C] (gate order r | z | n) and the state h [N, C] fp32 — mpnn.py:160-161; `out` is
    h_new in the dtype of gi (the tensor the next layer reads).  Backward recomputes the gates (csrc/gru.hip)."""

    @staticmethod
    def forward(ctx, gi, gh, h):
        N, C3 = gi.shape
        C = C3 // 3
        gi, gh, h = gi.contiguous(), gh.contiguous(), h.contiguous()
        h_new = torch.empty((N, C), dtype=torch.float32, device=gi.device)
        lp = gi.dtype != torch.float32
        out = torch.empty((N, C), dtype=gi.dtype, device=gi.device) if lp else None
        check(lib().mdl_gru_gates_fwd(ptr(gi), ptr(gh), ptr(h), ptr(h_new), ptr(out), N, C, dtype_code(gi), stream()), "mdl_gru_gates_fwd")
        ctx.save_for_backward(gi, gh, h)
        ctx.lp = lp
        if lp:
            return h_new, out
        dummy = h_new.new_empty(0)            # (fp32: callers use the first output for both roles — gru_gates below)
        ctx.mark_non_differentiable(dummy)
        return h_new, dummy

    @staticmethod
    def backward(ctx, g_h, g_out):
        gi, gh, h = ctx.saved_tensors
        N, C3 = gi.shape
        C = C3 // 3
        if not ctx.lp:
            g_out = None
        g_h = None if g_h is None else g_h.contiguous().float()
        g_out = None if g_out is None else g_out.contiguous().to(gi.dtype)
        if g_h is None and g_out is None:
            return None, None, None
        dgi, dgh = torch.empty_like(gi), torch.empty_like(gh)
        dh = torch.empty_like(h)
        check(lib().mdl_gru_gates_bwd(ptr(gi), ptr(gh), ptr(h), ptr(g_h), ptr(g_out), ptr(dgi), ptr(dgh), ptr(dh), N, C,
                                      dtype_code(gi), stream()), "mdl_gru_gates_bwd")
        return dgi, dgh, dh


def gru_gates_ok(gi, gh, h):
    return (gi.is_cuda and gi.dim() == 2 and gi.shape == gh.shape and gi.dtype == gh.dtype and gi.dtype in (torch.float32, torch.bfloat16)
            and gi.shape[1] % 3 == 0 and h.dtype == torch.float32 and h.shape == (gi.shape[0], gi.shape[1] // 3) and gi.shape[0] > 0)


def gru_gates(gi, gh, h):
    """One GRU step's gates: returns (h_new [N, C] fp32, out [N, C] in gi's dtype — the same tensor as h_new for fp32)."""
    h_new, out = _GRUGates.apply(gi, gh, h)
    return (h_new, out) if gi.dtype != torch.float32 else (h_new, h_new)


# ------------------------------------------------------------------------------------------------
# Set2Set readout: every processing step in one launch per direction (csrc/set2set.hip)
# ------------------------------------------------------------------------------------------------
_SET2SET_FUSED = True


class _Set2Set(torch.autograd.Function):
    """q*_T [S, 2C] fp32 of Set2Set with a one-layer LSTM (cgcnn.py:112-119 via torch_geometric.nn.Set2Set) from x [N, C] and the
    segment index of its sorted node -> graph map.  Forward: mdl_set2set_fwd (all steps; with the activated gates, c, q, r and the
    attention weights kept when a gradient is wanted).  Backward: mdl_set2set_bwd (dx, written once, zeros outside the segments,
    and dG [T, S, 4C]) and the parameter gradients as dense products over the stacked rows: dW_ih = dG[1:]^T [q | r][:-1],
    dW_hh = dG[1:]^T q[:-1] (h = q: the left half of dW_ih), db_ih = db_hh = column sums of dG (fp32 operands: the library's
    GEMM — the TN kernel of this package takes bf16 operands only)."""

    @staticmethod
    def forward(ctx, x, si, w_ih, w_hh, b_ih, b_hh, steps):
        N, C = x.shape
        S, T = si.N, int(steps)
        x = x.contiguous()
        w_ih, w_hh, b_ih, b_hh = w_ih.contiguous(), w_hh.contiguous(), b_ih.contiguous(), b_hh.contiguous()
        dev = x.device
        out = torch.empty((S, 2 * C), dtype=torch.float32, device=dev)
        gates = cqr = a = None
        if any(ctx.needs_input_grad):
            gates = torch.empty((T, S, 4 * C), dtype=torch.float32, device=dev)
            cqr = torch.empty((3, T, S, C), dtype=torch.float32, device=dev)
            a = torch.empty((T, N), dtype=torch.float32, device=dev)
        c, q, r = (cqr[0], cqr[1], cqr[2]) if cqr is not None else (None, None, None)
        check(lib().mdl_set2set_fwd(ptr(x), ptr(si.rowptr), ptr(w_ih), ptr(w_hh), ptr(b_ih), ptr(b_hh), ptr(out), ptr(gates), ptr(c),
                                    ptr(q), ptr(r), ptr(a), N, S, C, T, dtype_code(x), stream()), "mdl_set2set_fwd")
        ctx.si, ctx.T = si, T
        if gates is not None:
            ctx.save_for_backward(x, w_ih, w_hh, gates, cqr, a)
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g):
        x, w_ih, w_hh, gates, cqr, a = ctx.saved_tensors
        si, T = ctx.si, ctx.T
        N, C = x.shape
        S = si.N
        need = ctx.needs_input_grad
        g = g.contiguous().float()
        dx = torch.empty_like(x) if need[0] else None
        da = torch.empty((T, N), dtype=torch.float32, device=x.device) if need[0] else None
        dG = torch.empty((T, S, 4 * C), dtype=torch.float32, device=x.device)
        check(lib().mdl_set2set_bwd(ptr(x), ptr(si.rowptr), ptr(w_ih), ptr(w_hh), ptr(g), ptr(gates), ptr(cqr[0]), ptr(cqr[1]),
                                    ptr(cqr[2]), ptr(a), ptr(da), ptr(dx), ptr(dG), N, S, C, T, dtype_code(x), stream()), "mdl_set2set_bwd")
        dw_ih = dw_hh = db_ih = db_hh = None
        if need[2] or need[3]:
            if T > 1 and S > 0:               # (the t = 1 terms vanish: q*_0 = h_0 = 0)
                qr = torch.cat([cqr[1, :T - 1], cqr[2, :T - 1]], dim=-1).view((T - 1) * S, 2 * C)
                dw_ih = dG[1:].view((T - 1) * S, 4 * C).t().mm(qr)
            else:
                dw_ih = torch.zeros((4 * C, 2 * C), dtype=torch.float32, device=x.device)
            dw_hh = dw_ih[:, :C].contiguous() if need[3] else None
            dw_ih = dw_ih if need[2] else None
        if need[4] or need[5]:
            db = dG.view(T * S, 4 * C).sum(dim=0)
            db_ih = db if need[4] else None
            db_hh = (db.clone() if need[4] else db) if need[5] else None
        return dx, None, dw_ih, dw_hh, db_ih, db_hh, None


def set2set_fused_ok(x, steps):
    """ops.set2set takes this readout: 2-D fp32 / bf16 rows on a HIP device of a width and step count the kernels have (1 <= C <= 128,
    1 <= T <= 8 — mdl_set2set_supported)"""
    return (x.is_cuda and x.dim() == 2 and x.dtype in (torch.float32, torch.bfloat16) and x.shape[1] >= 1
            and bool(lib().mdl_set2set_supported(int(x.shape[1]), int(steps), dtype_code(x))))


def set2set(x, seg_index, w_ih, w_hh, b_ih, b_hh, steps):
    """Set2Set (A.6) of x [N, C] over the segments of `seg_index` — the index `scatter(x, batch, 0, size, ..., assume_sorted=True)`
    would use (`_seg_index(batch, size, True)`, or make_seg_index) — with the parameters of torch.nn.LSTM(2C, C) (fp32,
    `weight_ih_l0` [4C, 2C], `weight_hh_l0` [4C, C], the two biases [4C]) and `steps` processing steps: q*_T [S, 2C] fp32.
    One autograd node, differentiable in x and the four parameters; rows of x outside every segment get a zero gradient."""
    require_hip(x, w_ih, w_hh, b_ih, b_hh)
    if not set2set_fused_ok(x, steps):
        raise MdlError("set2set: needs 2-D fp32 / bf16 rows of 1..128 channels and 1..8 steps (got %s %s, %d steps)"
                       % (tuple(x.shape), x.dtype, steps))
    C = x.shape[1]
    for name, t, shape in (("w_ih", w_ih, (4 * C, 2 * C)), ("w_hh", w_hh, (4 * C, C)), ("b_ih", b_ih, (4 * C,)), ("b_hh", b_hh, (4 * C,))):
        if t.dtype != torch.float32 or tuple(t.shape) != shape:
            raise MdlError("set2set: %s must be fp32 %s (got %s %s)" % (name, shape, t.dtype, tuple(t.shape)))
    if seg_index.perm is not None or seg_index.E != x.shape[0]:
        raise MdlError("set2set: the segment index must be that of a sorted index over the %d rows of x" % x.shape[0])
    return _Set2Set.apply(x, seg_index, w_ih, w_hh, b_ih, b_hh, int(steps))


# ------------------------------------------------------------------------------------------------
# training loss: value and gradient in one launch
# ------------------------------------------------------------------------------------------------
_UNIT = {}


def unit_grad(device):
    """The constant fp32 scalar 1.0 on `device`, for `loss.backward(gradient=ops.unit_grad(dev))`: autograd's own root gradient is a
    fresh ones_like (a fill launch) that the fused loss then multiplies its stored gradient with (a second one); the loss node
    recognises THIS tensor by its address and hands its gradient on as it is.  Never written to."""
    device = torch.device(device)
    key = (device.type, device.index if device.index is not None else torch.cuda.current_device())
    t = _UNIT.get(key)
    if t is None:
        t = _UNIT[key] = torch.ones((), dtype=torch.float32, device=device)
    return t


def backward(loss):
    """loss.backward() with the constant unit root gradient (see unit_grad) when the loss is an fp32 device scalar"""
    if loss.is_cuda and loss.dtype == torch.float32 and loss.dim() == 0:
        loss.backward(gradient=unit_grad(loss.device))
    else:
        loss.backward()


def _is_unit(g):
    t = _UNIT.get((g.device.type, g.device.index))
    return t is not None and g.data_ptr() == t.data_ptr() and g.dim() == 0


class _FusedLoss(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, kind, rows, buf):
        p = pred.contiguous()
        y = target.contiguous()
        # loss | gradient; buf: the caller's persistent fp32 buffer of >= 1 + numel elements (GraphedStep reads the loss value of
        # a replayed step from its first element — no copy launch at the end of the step)
        out = torch.empty(1 + p.numel(), dtype=torch.float32, device=p.device) if buf is None else buf[:1 + p.numel()]
        if rows is None:
            check(lib().mdl_loss_fwd_bwd(ptr(p), ptr(y), p.numel(), kind, ptr(out), ptr(out[1:]), stream()), "mdl_loss_fwd_bwd")
        else:
            check(lib().mdl_loss_fwd_bwd_rows(ptr(p), ptr(y), int(rows), p.numel(), kind, ptr(out), ptr(out[1:]), stream()),
                  "mdl_loss_fwd_bwd_rows")
        ctx.save_for_backward(out)
        ctx.shape = tuple(pred.shape)
        return out[0]

    @staticmethod
    def backward(ctx, g):
        (out,) = ctx.saved_tensors
        grad = out[1:] if _is_unit(g) else out[1:] * g
        return grad.view(ctx.shape), None, None, None, None


def loss(name, pred, target, rows=None, buf=None):
    """getattr(F, name)(pred, target) as the reference's train() evaluates it (training.py:44-47).  l1_loss / mse_loss on
    fp32 HIP tensors of equal shape compute the value and d loss / d pred in one launch; anything else is torch's.
    rows: the loss of pred[:rows] against target (`rows` elements) with the gradient of the remaining predictions written as
    zeros by the same launch (the padded static batch's dummy graph) — no slice node between the model and the loss.
    buf: optional persistent fp32 device buffer (>= 1 + pred.numel() elements, contiguous) that receives [loss | gradient] when the
    fused kernel runs; the returned loss is then a view of buf[0]."""
    if buf is not None and not (buf.is_cuda and buf.dtype == torch.float32 and buf.is_contiguous() and buf.dim() == 1
                                and buf.numel() >= 1 + pred.numel() and buf.device == pred.device):
        buf = None
    kind = {"l1_loss": 0, "mse_loss": 1}.get(name)
    if rows is not None:
        rows = int(rows)
        if (kind is not None and pred.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32 and pred.dim() == 1
                and target.dim() == 1 and target.numel() == rows and 1 <= rows <= pred.numel() and not target.requires_grad):
            return _FusedLoss.apply(pred, target, kind, rows, buf)
        pred = pred[:rows]
    if (kind is not None and pred.is_cuda and pred.dtype == torch.float32 and target.dtype == torch.float32
            and pred.shape == target.shape and pred.numel() >= 1 and not target.requires_grad):
        return _FusedLoss.apply(pred, target, kind, None, buf)
    return getattr(torch.nn.functional, name)(pred, target)


# ------------------------------------------------------------------------------------------------
# training-mode BatchNorm1d over rows (HIP streams instead of four slow library passes)
# ------------------------------------------------------------------------------------------------
def bn_supported(x):
    if not (x.is_cuda and x.dim() == 2 and x.is_contiguous() and x.dtype in (torch.float32, torch.bfloat16)):
        return False
    c = x.shape[1]
    w = 8 if (x.dtype == torch.bfloat16 and c % 8 == 0) else 4          # 16-byte vectors, or 4 bf16 (C = 100, 150)
    # (N == 1 in training mode goes to the library path, which raises like torch does)
    return x.shape[0] >= 2 and c % 4 == 0 and 4 <= c <= 256 and x.data_ptr() % (w * x.element_size()) == 0


# Static (padded) batches of the HIP-graph path: the tensors hold `capacity` rows, the first *n_rows (a device scalar)
# exist.  Row-count-dependent kernels (BatchNorm) read it on the device.  None = every row exists.
_TRUE_ROWS = None


def _true_rows_for(nrows):
    """device row count for a tensor with `nrows` rows (None = all rows exist)"""
    tr = _TRUE_ROWS
    if tr is None:
        return None
    if isinstance(tr, dict):
        return tr.get(int(nrows))
    return tr


class true_rows:
    """`with ops.true_rows(n_dev):` — n_dev: int64 device tensor with one element, the number of rows that exist; or a dict
    {rows of the padded tensor: device scalar} when node-, edge- and graph-level tensors are padded to different capacities
    (a tensor whose row count is not in the dict is taken as complete)."""

    def __init__(self, n_dev):
        self.n_dev = n_dev

    def __enter__(self):
        global _TRUE_ROWS
        self.prev, _TRUE_ROWS = _TRUE_ROWS, self.n_dev
        return self

    def __exit__(self, *exc):
        global _TRUE_ROWS
        _TRUE_ROWS = self.prev
        return False


def bn_sums_rows():
    """rows of the BatchNorm kernels' sums buffer (replicas + totals)"""
    return int(lib().mdl_bn_sums_rows())


class _BatchNormTrain(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, weight, bias, running_mean, running_var, eps, momentum):
        N, C = x.shape
        dt = dtype_code(x)
        R = lib().mdl_bn_sums_rows()
        buf = _zeros_step((R + 2, C), x.device)                               # rows 0..R-1: sums (copies + totals) | save
        sums, save = buf[:R], buf[-2:]
        gw, gb = _f32c(weight), _f32c(bias)
        y = torch.empty_like(x)
        nd = _true_rows_for(N)
        # (statistics + apply as ONE launch for few rows was built and measured slower at the reference's batch size — 0.54 vs
        # 0.49 ms/step: C / 8 workgroups walking all rows twice are a longer dependent chain than two wide launches;
        # experiments/patches/bn_one_launch.patch)
        check(lib().mdl_bn_stats_n(ptr(x), ptr(sums), N, C, ptr(nd), dt | _dflag(), stream()), "mdl_bn_stats")
        check(lib().mdl_bn_apply_n(ptr(x), ptr(sums), ptr(gw), ptr(gb), ptr(save), ptr(running_mean), ptr(running_var),
                                   ptr(y), N, C, float(eps), float(momentum), ptr(nd), dt, stream()), "mdl_bn_apply")
        ctx.n_dev = nd
        ctx.save_for_backward(x, save, gw)
        ctx.has = (weight is not None, bias is not None)
        ctx.wdt = None if weight is None else weight.dtype
        return y

    @staticmethod
    def backward(ctx, dy):
        x, save, gw = ctx.saved_tensors
        N, C = x.shape
        dy = dy.contiguous()
        dt = dtype_code(x)
        R = lib().mdl_bn_sums_rows()
        sums = _zeros_grad(R * C, x.device).view(R, C)                       # (the step's GRADIENT arena, never reused: the totals
        dx = torch.empty_like(x)                                              # rows are returned as parameter gradients)
        nd = ctx.n_dev
        check(lib().mdl_bn_bwd_stats_n(ptr(dy), ptr(x), ptr(save), ptr(sums), N, C, ptr(nd), dt | _dflag(), stream()), "mdl_bn_bwd_stats")
        check(lib().mdl_bn_bwd_apply_n(ptr(dy), ptr(x), ptr(save), ptr(sums), ptr(gw), ptr(dx), N, C, ptr(nd), dt, stream()),
              "mdl_bn_bwd_apply")
        dgamma = sums[R - 1].to(ctx.wdt) if ctx.has[0] else None          # totals row pair published by bwd_apply
        dbeta = sums[R - 2].to(ctx.wdt) if ctx.has[1] else None
        return dx, dgamma, dbeta, None, None, None, None


class _LinearReluBN(torch.autograd.Function):
    """BatchNorm1d(relu(x W^T + b [+ sum_i table_i[idx_i]])) in training mode as ONE autograd node (the layer order of the
    reference's MEGNet blocks, megnet.py:41-56).  Forward: the streaming dense layer (K6 when tables are gathered), then the
    BatchNorm statistics and apply kernels.  Backward: the BatchNorm backward's apply pass also takes the ReLU mask (it reads the
    ReLU output anyway: mdl_bn_bwd_apply_relu_n), so what it writes is the gradient w.r.t. the pre-activation — the dense
    backward behind it runs without an activation staging (no second read of the output rows, the faster 8-wave form) and the
    gathered tables' gradients are segment sums of the same rows (no separate masked copy).  (Folding the BatchNorm apply
    into the dense backward's staging instead was measured no faster: experiments/patches/linear_relu_bn_fold.patch.)"""

    @staticmethod
    def forward(ctx, x, weight, bias, w_lp, b_lp, bn_w, bn_b, rm, rv, eps, momentum, idx, *tables):
        w, b = _wb(x, weight, bias, w_lp, b_lp)
        N, K = x.shape
        M = weight.shape[0]
        dt = dtype_code(x)
        y = torch.empty((N, M), dtype=x.dtype, device=x.device)
        targs, tabs = _table_args(idx, tables)
        R = lib().mdl_bn_sums_rows()
        buf = _zeros_step((R + 3, M), x.device)                       # sums | the epilogue's shift row | save
        sums, save = buf[:R], buf[R + 1:]
        nd = _true_rows_for(N)
        # the statistics of the BatchNorm ride in the dense layer's epilogue (per-column sums of the rounded outputs about output
        # row 0, which the kernel evaluates for itself and leaves in the shift row) —
        # except in deterministic mode, where the one-workgroup statistics kernel gives the run-to-run reproducible sums
        in_epilogue = not _DET and len(tables) in (0, 2) and K <= 160
        if in_epilogue:
            launch = lambda: lib().mdl_linear_act_stats(ptr(x), ptr(w), ptr(b), *targs, ptr(y), N, K, M, 1, ptr(sums), ptr(nd), dt,
                                                        stream())
            # (bench.py's K6 events: the edge block's first layer only — the launches with gathered tables)
            check(_launch_timed("edge_linear", launch) if tables else launch(), "mdl_linear_act_stats")
        elif tables:
            check(_launch_timed("edge_linear", lambda: lib().mdl_linear_gather_act(
                ptr(x), ptr(w), ptr(b), *targs, ptr(y), N, K, M, 1, dt, stream())), "mdl_linear_gather_act")
        else:
            check(lib().mdl_linear_act(ptr(x), ptr(w), ptr(b), ptr(y), N, K, M, 1, dt, stream()), "mdl_linear_act")
        gw, gb = _f32c(bn_w), _f32c(bn_b)
        z = torch.empty_like(y)
        if not in_epilogue:
            check(lib().mdl_bn_stats_n(ptr(y), ptr(sums), N, M, ptr(nd), dt | _dflag(), stream()), "mdl_bn_stats")
        check(lib().mdl_bn_apply_n(ptr(y), ptr(sums), ptr(gw), ptr(gb), ptr(save), ptr(rm), ptr(rv), ptr(z), N, M, float(eps),
                                   float(momentum), ptr(nd), dt | (_lib.MDL_BN_SHIFT_ROW if in_epilogue else 0), stream()),
              "mdl_bn_apply")
        ctx.save_for_backward(x, w, y, save, gw)
        ctx.n_dev, ctx.idx, ctx.rows = nd, list(idx), [None if t is None else t.shape[0] for t in tabs]
        ctx.wdtype, ctx.has_bias, ctx.shape = weight.dtype, bias is not None, tuple(weight.shape)
        ctx.bn_has = (bn_w is not None, bn_b is not None)
        ctx.bn_wdt = None if bn_w is None else bn_w.dtype
        return z

    @staticmethod
    def backward(ctx, gz):
        x, w, y, save, gw = ctx.saved_tensors
        N, M = y.shape
        gz = gz.contiguous()
        dt = dtype_code(x)
        R = lib().mdl_bn_sums_rows()
        sums = _zeros_grad(R * M, x.device).view(R, M)
        gp = torch.empty_like(y)                                                 # gradient w.r.t. the Linear's output (pre-activation)
        check(lib().mdl_bn_bwd_stats_n(ptr(gz), ptr(y), ptr(save), ptr(sums), N, M, ptr(ctx.n_dev), dt | _dflag(), stream()),
              "mdl_bn_bwd_stats")
        check(lib().mdl_bn_bwd_apply_relu_n(ptr(gz), ptr(y), ptr(save), ptr(sums), ptr(gw), ptr(gp), N, M, ptr(ctx.n_dev), dt,
                                            stream()), "mdl_bn_bwd_apply_relu")
        dgamma = sums[R - 1].to(ctx.bn_wdt) if ctx.bn_has[0] else None
        dbeta = sums[R - 2].to(ctx.bn_wdt) if ctx.bn_has[1] else None
        dx, dw, db, _ = _linear_backward(ctx, gp, x, w, 0, None, 0, False)      # (gp is w.r.t. the pre-activation: no activation left)
        return (dx, dw, db, None, None, dgamma, dbeta) + (None,) * 5 + _table_grads(gp, ctx.idx, ctx.rows, ctx.needs_input_grad[12:])


def linear_relu_bn_ok(x, weight, has_bias, gathered=None):
    """The fused Linear -> ReLU -> BatchNorm1d(train) node takes this layer: bf16 rows with a gradient, the dense-backward
    shapes (even widths in [34, 160], not both above 128), at most three gathered tables."""
    M, K = weight.shape
    return (_DENSE_BWD and x.dtype == torch.bfloat16 and x.is_cuda and x.dim() == 2 and x.is_contiguous() and x.shape[0] >= _DENSE_MIN_ROWS
            and x.requires_grad and torch.is_grad_enabled() and weight.requires_grad
            and _relu_bn_shape_ok(M, K, has_bias, len(gathered or ())) and x.data_ptr() % 16 == 0)


def linear_relu_bn(x, weight, bias, lowp, bn_weight, bn_bias, running_mean, running_var, eps, momentum, gathered=None):
    """BatchNorm1d(relu(F.linear(x, weight, bias) + sum_i table_i[index_i])) with batch statistics (callers check
    linear_relu_bn_ok); `gathered` = [(table [rows, M], index [N] int), ...]."""
    gathered = gathered or []
    idx = [ix if ix.dtype == torch.int32 else ix.to(torch.int32) for _, ix in gathered]
    return _LinearReluBN.apply(x, weight, bias, *_lowp_pair(lowp, x), bn_weight, bn_bias, running_mean, running_var, eps, momentum, idx,
                               *[t.to(x.dtype) for t, _ in gathered])


def batch_norm_train(x, weight, bias, running_mean, running_var, eps=1e-5, momentum=0.1):
    return _BatchNormTrain.apply(x, weight, bias, running_mean, running_var, eps, momentum)


# ------------------------------------------------------------------------------------------------
# N2 — crystal graphs from positions (process.py:258-305,540-559; csrc/graph_build.hip)
# ------------------------------------------------------------------------------------------------
GRAPH_MAX_NEIGHBORS = 64


def _graph_args(pos, node_ptr, cell, pbc):
    require_hip(pos, node_ptr, cell, pbc)
    if pos.dtype != torch.float64 or pos.dim() != 2 or pos.shape[1] != 3:
        raise MdlError("build_graphs: pos must be [N, 3] float64 (got %s %s)" % (tuple(pos.shape), pos.dtype))
    if node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 2:
        raise MdlError("build_graphs: node_ptr must be [G + 1] int64 with G >= 1")
    G = node_ptr.numel() - 1
    if cell.dtype != torch.float64 or tuple(cell.shape) != (G, 3, 3):
        raise MdlError("build_graphs: cell must be [G, 3, 3] float64 (got %s %s)" % (tuple(cell.shape), cell.dtype))
    if pbc.dim() == 2 and tuple(pbc.shape) == (G, 3):                # [G, 3] booleans -> bitmask
        pbc = (pbc.to(torch.int32) * torch.tensor([1, 2, 4], dtype=torch.int32, device=pbc.device)).sum(1, dtype=torch.int32)
    if pbc.dtype != torch.int32 or tuple(pbc.shape) != (G,):
        raise MdlError("build_graphs: pbc must be a [G] int32 bitmask or [G, 3] booleans")
    return pos.contiguous(), node_ptr.contiguous(), cell.contiguous(), pbc.contiguous(), G


def _build_graphs_launch(pos, node_ptr, cell, pbc, G, radius, max_neighbors):
    """The HIP launches alone (no host synchronisation): edge arrays at their bound N (k + 1), edge_ptr [G + 1] on the device."""
    N, k, dev = pos.shape[0], int(max_neighbors), pos.device
    nbytes = lib().mdl_graph_workspace_bytes(N, G, k)
    ws = torch.empty(max(nbytes, 1), dtype=torch.uint8, device=dev)
    cap = N * (k + 1) if 1 <= k <= GRAPH_MAX_NEIGHBORS else 1
    edge_ptr = torch.empty(G + 1, dtype=torch.int64, device=dev)
    src = torch.empty(cap, dtype=torch.int32, device=dev)
    tgt = torch.empty(cap, dtype=torch.int32, device=dev)
    dist = torch.empty(cap, dtype=torch.float32, device=dev)
    out_deg = torch.empty(N, dtype=torch.int32, device=dev)
    check(lib().mdl_graph_build(ptr(pos), ptr(node_ptr), ptr(cell), ptr(pbc), N, G, float(radius), k, ptr(edge_ptr), ptr(src),
                                ptr(tgt), ptr(dist), ptr(out_deg), cap, ptr(ws), nbytes, stream()), "mdl_graph_build")
    return edge_ptr, src, tgt, dist, out_deg


def build_graphs(pos, node_ptr, cell, pbc, radius=8.0, max_neighbors=12):
    """Graphs of G structures at once, the reference's rule (process.py:258-305: minimum-image distances, at most
    max_neighbors nearest within radius per source row, self loops) on the device.
      pos [N, 3] float64; node_ptr [G + 1] int64 (atoms of structure g: node_ptr[g]:node_ptr[g + 1]); cell [G, 3, 3] float64;
      pbc [G] int32 bitmask (bit a: axis a periodic) or [G, 3] booleans.
    Returns device tensors (edge_ptr [G + 1] int64, src [E] int32, tgt [E] int32, dist [E] float32, out_deg [N] int32): per graph
    the edges CSR by target with graph-local node ids (in-edges by ascending source, then the self loop), dist the fp32
    minimum-image distance, out_deg the out-degree including the self loop — exactly what process.from_structures builds on
    the host.  Validating node_ptr and trimming the edges to E read two numbers back (two host synchronisations)."""
    pos, node_ptr, cell, pbc, G = _graph_args(pos, node_ptr, cell, pbc)
    N = pos.shape[0]
    if N < 1:
        raise MdlError("build_graphs: no atoms")
    bad = (node_ptr[0] != 0) | (node_ptr[-1] != N) | (node_ptr[1:] < node_ptr[:-1]).any()
    if bool(bad):
        raise MdlError("build_graphs: node_ptr must start at 0, be non-decreasing and end at N = %d" % N)
    edge_ptr, src, tgt, dist, out_deg = _build_graphs_launch(pos, node_ptr, cell, pbc, G, radius, max_neighbors)
    E = int(edge_ptr[-1])
    return edge_ptr, src[:E], tgt[:E], dist[:E], out_deg


# ------------------------------------------------------------------------------------------------
# Edge geometry: distances of given edges as a differentiable function of the positions (csrc/edge_geom.hip)
# ------------------------------------------------------------------------------------------------
class _EdgeVectors(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pos, node_ptr, cell, pbc, src, tgt, csr):
        N, G, E = pos.shape[0], node_ptr.numel() - 1, src.numel()
        dist = torch.empty(E, dtype=torch.float32, device=pos.device)
        u = torch.empty((E, 3), dtype=torch.float32, device=pos.device)
        nbytes = lib().mdl_edge_geometry_workspace_bytes(G)
        ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=pos.device)
        check(lib().mdl_edge_geometry_fwd(ptr(pos), ptr(node_ptr), ptr(cell), ptr(pbc), N, G, ptr(src), ptr(tgt), E, ptr(dist), ptr(u),
                                          ptr(ws), nbytes, stream()), "mdl_edge_geometry_fwd")
        ctx.save_for_backward(u, src, tgt)
        ctx.csr, ctx.N, ctx.pos_dtype = csr, N, pos.dtype
        ctx.mark_non_differentiable(u)
        return dist, u

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g_dist, _g_u):
        u, src, tgt = ctx.saved_tensors
        csr = ctx.csr
        if csr is None:                                    # one sort by target and one by source, both stable: deterministic
            csr = build_csr(torch.stack([src, tgt]), ctx.N)
        rowptr_s, _, eid_s, _ = csr.transposed()
        dpos = torch.empty((ctx.N, 3), dtype=torch.float32, device=u.device)
        check(lib().mdl_edge_geometry_bwd(ptr(g_dist.float().contiguous()), ptr(u), ptr(csr.rowptr), ptr(csr.eperm), ptr(rowptr_s), ptr(eid_s),
                                          ctx.N, u.shape[0], ptr(dpos), stream()), "mdl_edge_geometry_bwd")
        return dpos.to(ctx.pos_dtype), None, None, None, None, None, None


def edge_vectors(pos, node_ptr, cell, pbc, src, tgt, edge_ptr=None, csr=None, return_unit=False):
    """Minimum-image distances of GIVEN edges, differentiable (first order) w.r.t. the positions.
      pos / node_ptr / cell / pbc as in build_graphs; src / tgt [E] int32: edges src -> tgt inside a structure.  With edge_ptr
      ([G + 1] int64, as build_graphs returns it) the ids are graph-local, otherwise batch-global.
    Returns dist [E] fp32 — for the edges build_graphs returned, bitwise the dist it returned (the same device code chooses the
    image: reduced cell, completed basis, rint wrap, +-1 images) — and with return_unit=True also u [E, 3] fp32, the unit vector
    of the displacement p_tgt - p_src + shift (0 for self loops and coincident atoms; carries no gradient).
    The backward is dpos[tgt] += g u, dpos[src] -= g u as two segmented sums (by target and by source: no atomics, bitwise
    repeatable).  The image shifts and the cell are held fixed: there is no gradient w.r.t. `cell` under autograd; the strain
    gradient (stress) comes from the gradient w.r.t. `dist` through edge_strain_grad.
    csr: an EdgeCSR of the batch-global edge list, if the caller has one (saves the backward its two sorts)."""
    pos, node_ptr, cell, pbc, G = _graph_args(pos, node_ptr, cell, pbc)
    require_hip(src, tgt)
    if src.dtype != torch.int32 or tgt.dtype != torch.int32 or src.shape != tgt.shape or src.dim() != 1:
        raise MdlError("edge_vectors: src / tgt must be [E] int32")
    if pos.shape[0] < 1:
        raise MdlError("edge_vectors: no atoms")
    if edge_ptr is not None:
        shift = torch.repeat_interleave(node_ptr[:-1], edge_ptr[1:] - edge_ptr[:-1], output_size=src.numel()).to(torch.int32)
        src, tgt = src + shift, tgt + shift
    if csr is not None and (csr.N != pos.shape[0] or csr.E != src.numel()):
        raise MdlError("edge_vectors: csr does not match the edge list")
    dist, u = _EdgeVectors.apply(pos, node_ptr, cell, pbc, src.contiguous(), tgt.contiguous(), csr)
    return (dist, u) if return_unit else dist


def edge_strain_grad(g_dist, dist, u, node_ptr, csr=None, src=None, tgt=None, _slices=None):
    """Strain gradient of the energy per graph from the gradient w.r.t. the edge distances (csrc/edge_geom.hip).
      g_dist [E] = dE/d dist (what autograd hands to the backward of edge_vectors), dist [E] fp32 and u [E, 3] fp32 as
      edge_vectors(..., return_unit=True) returned them, node_ptr [G + 1] int64.
      csr: the EdgeCSR (by target) of the batch-global edge list; without one it is built from src / tgt [E] int32 (one stable
      sort, and one number read back for the atom count).
    Returns [G, 3, 3] fp32:  out[g] = sum_{e in g} g_e d_e u_e (x) u_e = dE/d eps of a homogeneous strain v -> (I + eps) v of the
    structure (positions, cell and image shifts together) at fixed neighbour lists — stress times volume, tensile positive.
    Symmetric to the bit, fp64 accumulation, no atomics: two calls give the same bits.  Not an autograd node: g_dist is a number."""
    require_hip(g_dist, dist, u, node_ptr)
    E = dist.numel()
    if dist.dtype != torch.float32 or dist.dim() != 1 or u.dtype != torch.float32 or tuple(u.shape) != (E, 3):
        raise MdlError("edge_strain_grad: dist must be [E] float32 and u [E, 3] float32 (got %s %s, %s %s)"
                       % (tuple(dist.shape), dist.dtype, tuple(u.shape), u.dtype))
    if not g_dist.is_floating_point() or tuple(g_dist.shape) != (E,):
        raise MdlError("edge_strain_grad: g_dist must be [E] floating point with E = %d (got %s %s)" % (E, tuple(g_dist.shape), g_dist.dtype))
    if node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 2:
        raise MdlError("edge_strain_grad: node_ptr must be [G + 1] int64 with G >= 1")
    if any(t.device != dist.device for t in (g_dist, u, node_ptr)):
        raise MdlError("edge_strain_grad: g_dist, dist, u and node_ptr must be on one device")
    if csr is None:
        if src is None or tgt is None:
            raise MdlError("edge_strain_grad: needs the EdgeCSR of the edge list, or src / tgt to build it")
        require_hip(src, tgt)
        if src.dtype != torch.int32 or tgt.dtype != torch.int32 or tuple(src.shape) != (E,) or tuple(tgt.shape) != (E,):
            raise MdlError("edge_strain_grad: src / tgt must be [E] int32")
        csr = build_csr(torch.stack([src, tgt]), int(node_ptr[-1]))
    if csr.E != E or csr.rowptr.device != dist.device:
        raise MdlError("edge_strain_grad: csr does not match the edge list")
    S = 0 if _slices is None else int(_slices)
    if _slices is not None and not 1 <= S <= 65536:
        raise MdlError("edge_strain_grad: _slices must be in [1, 65536] (got %d)" % S)
    G = node_ptr.numel() - 1
    out = torch.empty((G, 3, 3), dtype=torch.float32, device=dist.device)
    nbytes = lib().mdl_edge_strain_grad_workspace_bytes(G, E, S)
    ws = torch.empty(max(nbytes, 8), dtype=torch.uint8, device=dist.device)
    check(lib().mdl_edge_strain_grad(ptr(g_dist.detach().float().contiguous()), ptr(dist.detach().contiguous()), ptr(u.contiguous()),
                                     ptr(csr.rowptr), ptr(csr.eperm), ptr(node_ptr.contiguous()), csr.N, G, E, S, ptr(out), ptr(ws),
                                     nbytes, stream()), "mdl_edge_strain_grad")
    return out


# ------------------------------------------------------------------------------------------------
# Relaxation: one FIRE update of a batch of structures in one launch (csrc/relax.hip)
# ------------------------------------------------------------------------------------------------
FIRE_CONSTANTS = {"n_min": 5, "f_inc": 1.1, "f_dec": 0.5, "alpha_start": 0.1, "f_alpha": 0.99, "dt_max": 1.0, "maxstep": 0.2}


class FireState:
    """Per-structure state of fire_step, [B] device tensors: dt, alpha float64; n_pos (steps with F.v > 0 in a row), steps (updates
    made) and done (the convergence latch) int32; fmax_seen float32, the max_i |F_i| every call writes."""

    __slots__ = ("dt", "alpha", "n_pos", "steps", "done", "fmax_seen")

    def __init__(self, dt, alpha, n_pos, steps, done, fmax_seen):
        self.dt, self.alpha, self.n_pos, self.steps, self.done, self.fmax_seen = dt, alpha, n_pos, steps, done, fmax_seen

    def clone(self):
        return FireState(*[getattr(self, k).clone() for k in self.__slots__])


def fire_state(B, dt=0.1, alpha=0.1, device=None):
    """A fresh FireState of B structures: time step dt, mixing alpha, no step made, nothing converged."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    zi = lambda: torch.zeros(int(B), dtype=torch.int32, device=dev)
    return FireState(torch.full((int(B),), float(dt), dtype=torch.float64, device=dev),
                     torch.full((int(B),), float(alpha), dtype=torch.float64, device=dev), zi(), zi(), zi(),
                     torch.zeros(int(B), dtype=torch.float32, device=dev))


class FireCellState:
    """Per-structure state of fire_cell_step: the FireState fields ([B]: dt, alpha, n_pos, steps, done, fmax_seen) and what the
    cell's degrees of freedom add — scaled [N, 3] float64 (s: pos_i = F s_i), deform [B, 3, 3] float64 (F: cell = cell0 F^T),
    vel_cell [B, 3, 3] float64 (the velocity of W = cell_factor F), cell0 [B, 3, 3] float64 (the cell at the start), cell_free [B]
    uint8, cell_factor [B] float64, smax_seen [B] float32 (max |dE/d eps| / volume, written by every call).  done: 0 moving,
    1 converged, 2 stopped by the trust region (|F - I| would have exceeded max_deform)."""

    __slots__ = FireState.__slots__ + ("scaled", "deform", "vel_cell", "cell0", "cell_free", "cell_factor", "smax_seen")

    def __init__(self, *fields):
        if len(fields) != len(self.__slots__):
            raise MdlError("FireCellState: %d fields (%s)" % (len(self.__slots__), ", ".join(self.__slots__)))
        for k, v in zip(self.__slots__, fields):
            setattr(self, k, v)

    def clone(self):
        return FireCellState(*[getattr(self, k).clone() for k in self.__slots__])


# (field, dtype, shape behind [B]) of the state: the first six are FireState's
_FIRE_CELL_FIELDS = (("dt", torch.float64, ()), ("alpha", torch.float64, ()), ("n_pos", torch.int32, ()), ("steps", torch.int32, ()),
                     ("done", torch.int32, ()), ("fmax_seen", torch.float32, ()), ("deform", torch.float64, (3, 3)),
                     ("vel_cell", torch.float64, (3, 3)), ("cell0", torch.float64, (3, 3)), ("cell_free", torch.uint8, ()),
                     ("cell_factor", torch.float64, ()), ("smax_seen", torch.float32, ()))
FIRE_CELL_CONSTANTS = dict(FIRE_CONSTANTS, max_deform=0.5)
# entry point -> (its constants, its state, what makes one, the state's [B, ...] fields)
_FIRE_KINDS = {"fire_step": (FIRE_CONSTANTS, FireState, "fire_state", _FIRE_CELL_FIELDS[:len(FireState.__slots__)]),
               "fire_cell_step": (FIRE_CELL_CONSTANTS, FireCellState, "fire_cell_state", _FIRE_CELL_FIELDS)}


class NebState:
    """State of neb_step for I images in B bands: the FireState fields, [B], one set per BAND (dt, alpha, n_pos, steps, done,
    fmax_seen: the largest per-atom |F_band| of the band); the layout — image_ptr [I + 1], band_ptr [B + 1], band_node_ptr [B + 1]
    (= image_ptr[band_ptr]: the atoms of a band) int64 and fixed [N] uint8 (the caller's mask OR every atom of an end image) —;
    and what every call writes: climber [B] int32 (the climbing image's index in the batch, -1: none), tangent_force [I] float64
    (F.t^, 0 for end images), seg_len [I] float64 (the distance to the image before; 0 for a band's first) and band_force [N, 3]
    float32 (the projected force the update used)."""

    __slots__ = FireState.__slots__ + ("image_ptr", "band_ptr", "band_node_ptr", "fixed", "climber", "tangent_force", "seg_len", "band_force")

    def __init__(self, *fields):
        if len(fields) != len(self.__slots__):
            raise MdlError("NebState: %d fields (%s)" % (len(self.__slots__), ", ".join(self.__slots__)))
        for k, v in zip(self.__slots__, fields):
            setattr(self, k, v)

    def clone(self):
        return NebState(*[getattr(self, k).clone() for k in self.__slots__])


_FIRE_KINDS["neb_step"] = (FIRE_CONSTANTS, NebState, "neb_state", _FIRE_CELL_FIELDS[:len(FireState.__slots__)])
# the fields NebState adds: (field, dtype, shape from (N, I, B))
_NEB_FIELDS = (("image_ptr", torch.int64, lambda N, I, B: (I + 1,)), ("band_ptr", torch.int64, lambda N, I, B: (B + 1,)),
               ("fixed", torch.uint8, lambda N, I, B: (N,)), ("climber", torch.int32, lambda N, I, B: (B,)),
               ("tangent_force", torch.float64, lambda N, I, B: (I,)), ("seg_len", torch.float64, lambda N, I, B: (I,)),
               ("band_force", torch.float32, lambda N, I, B: (N, 3)))


def _fire_args(who, pos, vel, force, node_ptr, state, bounds, fixed, constants, cell=None, strain_grad=None):
    """The argument checks of fire_step and fire_cell_step (`who`: the name every message starts with; cell and strain_grad belong
    to fire_cell_step alone; bounds: (name, a number or a [B] float64 tensor) each).  Returns (the constants with their defaults,
    N, B, the bounds as contiguous [B] float64 device tensors, fixed as contiguous uint8 or None)."""
    known, state_type, maker, fields = _FIRE_KINDS[who]
    unknown = set(constants) - set(known)
    if unknown:
        raise MdlError("%s: unknown constants %s (known: %s)" % (who, sorted(unknown), sorted(known)))
    c = dict(known, **constants)
    if not isinstance(state, state_type):
        raise MdlError("%s: state must be an ops.%s (ops.%s)" % (who, state_type.__name__, maker))
    with_cell = state_type is FireCellState
    require_hip(pos, cell, vel, force, strain_grad, node_ptr, fixed, *[getattr(state, k) for k in state_type.__slots__])
    N = pos.shape[0] if pos.dim() == 2 else -1
    for name, t in (("pos", pos), ("vel", vel)) + ((("state.scaled", state.scaled),) if with_cell else ()):
        if t.dtype != torch.float64 or tuple(t.shape) != (N, 3) or not t.is_contiguous():
            raise MdlError("%s: %s must be a contiguous [N, 3] float64 tensor (got %s %s)" % (who, name, tuple(t.shape), t.dtype))
    if force.dtype != torch.float32 or tuple(force.shape) != (N, 3):
        raise MdlError("%s: force must be [N, 3] float32 with N = %d (got %s %s)" % (who, N, tuple(force.shape), force.dtype))
    if node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 1:
        raise MdlError("%s: node_ptr must be [B + 1] int64" % who)
    B = node_ptr.numel() - 1
    if with_cell:
        if cell.dtype != torch.float64 or tuple(cell.shape) != (B, 3, 3) or not cell.is_contiguous():
            raise MdlError("%s: cell must be a contiguous [B, 3, 3] float64 tensor with B = %d (got %s %s)" % (who, B, tuple(cell.shape), cell.dtype))
        if strain_grad.dtype != torch.float32 or tuple(strain_grad.shape) != (B, 3, 3):
            raise MdlError("%s: strain_grad must be [B, 3, 3] float32 with B = %d (got %s %s)" % (who, B, tuple(strain_grad.shape), strain_grad.dtype))
    for k, dt_, tail in fields:
        t = getattr(state, k)
        if t.dtype != dt_ or tuple(t.shape) != (B,) + tail or not t.is_contiguous():
            raise MdlError("%s: state.%s must be a contiguous %s %s tensor with B = %d (got %s %s)" % (who, k, list((B,) + tail), dt_, B, tuple(t.shape), t.dtype))
    out = []
    for name, v in bounds:
        if torch.is_tensor(v):
            if v.dtype != torch.float64 or tuple(v.shape) != (B,):
                raise MdlError("%s: %s must be a number or a [B] float64 tensor with B = %d (got %s %s)" % (who, name, B, tuple(v.shape), v.dtype))
            require_hip(v)
            out.append(v.contiguous())
        else:
            out.append(torch.full((B,), float(v), dtype=torch.float64, device=pos.device))
    if fixed is not None:
        if fixed.dtype not in (torch.uint8, torch.bool) or tuple(fixed.shape) != (N,):
            raise MdlError("%s: fixed must be [N] uint8 or bool with N = %d (got %s %s)" % (who, N, tuple(fixed.shape), fixed.dtype))
        fixed = fixed.contiguous().view(torch.uint8)
    if any(t.device != pos.device for t in [vel, force, node_ptr, state.dt] + out + ([cell, strain_grad, state.scaled] if with_cell else [])):
        raise MdlError("%s: pos, the other tensors (%s among them) and the state must be on one device" % (who, ", ".join(n for n, _ in bounds)))
    return c, N, B, out, fixed


def fire_step(pos, vel, force, node_ptr, state, fmax, fixed=None, **constants):
    """One FIRE update (unit masses) of every structure of a batch, in place, in ONE launch.
      pos, vel [N, 3] float64 (updated in place: contiguous tensors), force [N, 3] float32, node_ptr [B + 1] int64, state a
      FireState of B structures (updated in place), fmax a number or a [B] float64 tensor, fixed [N] uint8 / bool or None
      (non-zero: the atom stays where it is), constants: any of FIRE_CONSTANTS (n_min, f_inc, f_dec, alpha_start, f_alpha,
      dt_max, maxstep).
    A structure whose largest per-atom force is below its fmax — or that converged in an earlier call, or has no force on a free
    atom — gets state.done = 1 and is otherwise left alone: positions, velocities and the rest of its state keep their bits.
    The others move as include/mdl_hip.h (mdl_fire_step) states it.  No host synchronisation, no atomics: two calls from the same
    inputs give the same bits.  Returns state."""
    c, N, B, (fmax,), fixed = _fire_args("fire_step", pos, vel, force, node_ptr, state, (("fmax", fmax),), fixed, constants)
    check(lib().mdl_fire_step(ptr(pos), ptr(vel), ptr(force.contiguous()), ptr(fixed), ptr(node_ptr.contiguous()), N, B, ptr(fmax),
                              ptr(state.dt), ptr(state.alpha), ptr(state.n_pos), ptr(state.steps), ptr(state.done), ptr(state.fmax_seen),
                              int(c["n_min"]), float(c["f_inc"]), float(c["f_dec"]), float(c["alpha_start"]), float(c["f_alpha"]),
                              float(c["dt_max"]), float(c["maxstep"]), None, None, 0, *([None] * 9), stream()), "mdl_fire_step")   # no band
    return state


def fire_cell_state(pos, cell, node_ptr, cell_free=None, cell_factor=None, dt=0.1, alpha=0.1):
    """A fresh FireCellState for the geometry (pos [N, 3], cell [B, 3, 3] float64, node_ptr [B + 1] int64, device tensors): s = a
    copy of pos, F = I, no velocity of the cell, cell0 = a copy of cell, nothing converged.  cell_free [B] (non-zero: the cell of
    the structure moves; default: every cell), cell_factor [B] > 0 (default max(1, atoms of the structure)): the cell's rows enter
    as W = cell_factor F, so a strain of eps moves the integrator's coordinates as far as moving cell_factor atoms by eps each."""
    require_hip(pos, cell, node_ptr)
    if pos.dtype != torch.float64 or pos.dim() != 2 or pos.shape[1] != 3:
        raise MdlError("fire_cell_state: pos must be [N, 3] float64 (got %s %s)" % (tuple(pos.shape), pos.dtype))
    if node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 1:
        raise MdlError("fire_cell_state: node_ptr must be [B + 1] int64")
    B, dev = node_ptr.numel() - 1, pos.device
    if cell.dtype != torch.float64 or tuple(cell.shape) != (B, 3, 3):
        raise MdlError("fire_cell_state: cell must be [B, 3, 3] float64 with B = %d (got %s %s)" % (B, tuple(cell.shape), cell.dtype))

    def per_structure(v, name, dtype):
        t = (v.detach() if torch.is_tensor(v) else torch.as_tensor(v)).to(dev)
        if tuple(t.shape) != (B,):
            raise MdlError("fire_cell_state: %s must be one value per structure, [%d] (got %s)" % (name, B, tuple(t.shape)))
        return (t != 0).to(torch.uint8) if dtype == torch.uint8 else t.to(dtype).contiguous()

    free = torch.ones(B, dtype=torch.uint8, device=dev) if cell_free is None else per_structure(cell_free, "cell_free", torch.uint8)
    if cell_factor is None:
        factor = (node_ptr[1:] - node_ptr[:-1]).clamp(min=1).to(torch.float64)
    else:
        factor = per_structure(cell_factor, "cell_factor", torch.float64)
        if not bool((factor > 0).all()):
            raise MdlError("fire_cell_state: cell_factor must be > 0")
    base = fire_state(B, dt, alpha, dev)
    return FireCellState(*[getattr(base, k) for k in FireState.__slots__], pos.detach().clone().contiguous(),
                         torch.eye(3, dtype=torch.float64, device=dev).repeat(B, 1, 1), torch.zeros(B, 3, 3, dtype=torch.float64, device=dev),
                         cell.detach().clone().contiguous(), free, factor, torch.zeros(B, dtype=torch.float32, device=dev))


def fire_cell_step(pos, cell, vel, force, strain_grad, node_ptr, state, fmax, smax, fixed=None, **constants):
    """One FIRE update (unit masses) over the atoms AND the cell of every structure of a batch, in place, in ONE launch.
      pos, vel [N, 3] float64 and cell [B, 3, 3] float64 (updated in place: contiguous tensors; vel is the velocity of the scaled
      rows s), force [N, 3] float32, strain_grad [B, 3, 3] float32 (dE/d eps, NOT divided by the volume: ForceField.evaluate(
      stress=True, volume_normalised=False)), node_ptr [B + 1] int64, state a FireCellState (updated in place), fmax, smax a number
      or a [B] float64 tensor each, fixed [N] uint8 / bool or None, constants: any of FIRE_CELL_CONSTANTS (FIRE_CONSTANTS and
      max_deform in (0, 1)).
    Coordinates, generalised forces, the convergence rule (max_i |F_i| < fmax AND, where the cell is free, max |dE/d eps| / volume <
    smax), the trust region (state.done = 2) and the frozen-cell case (the bits of fire_step) are stated in include/mdl_hip.h
    (mdl_fire_cell_step).  No host synchronisation, no atomics: two calls from the same inputs give the same bits.  Returns state."""
    c, N, B, (fmax, smax), fixed = _fire_args("fire_cell_step", pos, vel, force, node_ptr, state, (("fmax", fmax), ("smax", smax)), fixed,
                                              constants, cell, strain_grad)
    check(lib().mdl_fire_cell_step(ptr(pos), ptr(cell), ptr(state.scaled), ptr(state.deform), ptr(vel), ptr(state.vel_cell), ptr(force.contiguous()),
                                   ptr(strain_grad.contiguous()), ptr(state.cell0), ptr(fixed), ptr(state.cell_free), ptr(state.cell_factor),
                                   ptr(node_ptr.contiguous()), N, B, ptr(fmax), ptr(smax), ptr(state.dt), ptr(state.alpha),
                                   ptr(state.n_pos), ptr(state.steps), ptr(state.done), ptr(state.fmax_seen), ptr(state.smax_seen),
                                   int(c["n_min"]), float(c["f_inc"]), float(c["f_dec"]), float(c["alpha_start"]), float(c["f_alpha"]),
                                   float(c["dt_max"]), float(c["maxstep"]), float(c["max_deform"]), stream()), "mdl_fire_cell_step")
    return state


# ------------------------------------------------------------------------------------------------
# Nudged elastic band: the band force of every image (csrc/neb.hip), then FIRE over whole bands — the band mode of mdl_fire_step
# ------------------------------------------------------------------------------------------------
def neb_state(image_ptr, band_ptr, fixed=None, dt=0.1, alpha=0.1):
    """A fresh NebState for I images (the structures of a batch: image_ptr [I + 1] int64, their node_ptr) grouped into B bands
    (band_ptr [B + 1] int64: band b owns the consecutive images band_ptr[b] .. band_ptr[b + 1] - 1; its first and last image are
    its fixed end points), device tensors.  fixed [N] uint8 / bool or None: atoms that do not move in any image they are in.
    The layout is validated ONCE, here, with a host read: image_ptr starts at 0 and does not decrease, band_ptr does not decrease
    and spans 0 .. I, and the images of a band have equal atom counts."""
    who = "neb_state"
    require_hip(image_ptr, band_ptr, fixed)
    for name, t in (("image_ptr", image_ptr), ("band_ptr", band_ptr)):
        if t.dtype != torch.int64 or t.dim() != 1 or t.numel() < 1:
            raise MdlError("%s: %s must be a 1-d int64 tensor with at least one entry" % (who, name))
    if band_ptr.device != image_ptr.device:
        raise MdlError("%s: image_ptr and band_ptr must be on one device" % who)
    dev, I, B = image_ptr.device, image_ptr.numel() - 1, band_ptr.numel() - 1
    ip, bp = image_ptr.detach().cpu(), band_ptr.detach().cpu()               # the one host read
    if int(ip[0]) != 0 or bool((ip[1:] < ip[:-1]).any()):
        raise MdlError("%s: image_ptr must start at 0 and be non-decreasing" % who)
    if int(bp[0]) != 0 or int(bp[-1]) != I or bool((bp[1:] < bp[:-1]).any()):
        raise MdlError("%s: band_ptr must be non-decreasing and span 0 .. I = %d (got %d .. %d)" % (who, I, int(bp[0]), int(bp[-1])))
    N, counts = int(ip[-1]), ip[1:] - ip[:-1]
    ends = torch.zeros(N, dtype=torch.bool)
    for b in range(B):
        i0, i1 = int(bp[b]), int(bp[b + 1])
        if i1 > i0:
            if bool((counts[i0:i1] != counts[i0]).any()):
                raise MdlError("%s: the images of band %d have unequal atom counts %s" % (who, b, counts[i0:i1].tolist()))
            for s in (i0, i1 - 1):
                ends[int(ip[s]):int(ip[s + 1])] = True
    mask = ends.to(dev)
    if fixed is not None:
        if fixed.dtype not in (torch.uint8, torch.bool) or tuple(fixed.shape) != (N,):
            raise MdlError("%s: fixed must be [N] uint8 or bool with N = %d (got %s %s)" % (who, N, tuple(fixed.shape), fixed.dtype))
        if fixed.device != dev:
            raise MdlError("%s: fixed must be on the device of image_ptr" % who)
        mask = mask | (fixed != 0)
    base = fire_state(B, dt, alpha, dev)
    return NebState(*[getattr(base, k) for k in FireState.__slots__], image_ptr.detach().clone().contiguous(),
                    band_ptr.detach().clone().contiguous(), ip[bp].to(dev), mask.to(torch.uint8),
                    torch.full((B,), -1, dtype=torch.int32, device=dev), torch.zeros(I, dtype=torch.float64, device=dev),
                    torch.zeros(I, dtype=torch.float64, device=dev), torch.zeros((N, 3), dtype=torch.float32, device=dev))


def neb_step(pos, vel, force, energy, cell, pbc, state, fmax, spring=1.0, climb=True, **constants):
    """One nudged-elastic-band step of every band of a batch, in place, in ONE call: the band force of every image — improved
    tangent, springs along it, the climbing image turned uphill (include/mdl_hip.h, mdl_fire_step, band mode) — and then the FIRE
    update of fire_step over whole BANDS: one time step, one alpha, one F.v and one convergence latch per band; maxstep bounds the
    norm of the band's whole displacement.
      pos, vel [N, 3] float64 (updated in place: contiguous tensors), force [N, 3] float32 (the TRUE force) and energy [I] float32
      of the images, cell [I, 3, 3] float64 and pbc [I] int32 (bit a: axis a periodic; what ForceField.cell / .pbc hold), state a
      NebState (ops.neb_state; updated in place), fmax, spring a number or a [B] float64 tensor each, climb a number / bool or a
      [B] tensor (non-zero: the band's interior image of largest energy climbs), constants: any of FIRE_CONSTANTS.
    A band is converged once the largest per-atom |F_band| over all its images is below its fmax; it is then left alone as
    fire_step leaves a structure.  state.band_force, .tangent_force, .seg_len and .climber are written for every band, converged
    or not.  Displacements between neighbouring images are wrapped to their minimum image in the cell of the middle one: exact
    while no atom moves half a cell height or more between neighbours — the caller's condition.  Two stream-ordered launches, no
    host synchronisation, no atomics: two calls from the same inputs give the same bits, a band alone or in any batch.
    Returns state."""
    who = "neb_step"
    if not isinstance(state, NebState):
        raise MdlError("%s: state must be an ops.NebState (ops.neb_state)" % who)
    require_hip(energy, cell, pbc)
    c, N, B, (fmax, spring), fixed = _fire_args(who, pos, vel, force, state.band_node_ptr, state, (("fmax", fmax), ("spring", spring)),
                                                state.fixed, constants)
    I = state.image_ptr.numel() - 1
    for k, dt_, shape in _NEB_FIELDS:
        t = getattr(state, k)
        if t.dtype != dt_ or tuple(t.shape) != shape(N, I, B) or not t.is_contiguous():
            raise MdlError("%s: state.%s must be a contiguous %s %s tensor (got %s %s)" % (who, k, list(shape(N, I, B)), dt_, tuple(t.shape), t.dtype))
    for name, t, dt_, shape in (("energy", energy, torch.float32, (I,)), ("cell", cell, torch.float64, (I, 3, 3)), ("pbc", pbc, torch.int32, (I,))):
        if t.dtype != dt_ or tuple(t.shape) != shape:
            raise MdlError("%s: %s must be %s %s with I = %d images (got %s %s)" % (who, name, list(shape), dt_, I, tuple(t.shape), t.dtype))
    if torch.is_tensor(climb):
        if tuple(climb.shape) != (B,):
            raise MdlError("%s: climb must be a number or a [B] tensor with B = %d (got %s)" % (who, B, tuple(climb.shape)))
        require_hip(climb)
        climb = (climb != 0).to(torch.uint8)
    else:
        climb = torch.full((B,), 1 if climb else 0, dtype=torch.uint8, device=pos.device)
    if any(t.device != pos.device for t in (energy, cell, pbc, climb, state.image_ptr, state.band_ptr, state.band_force)):
        raise MdlError("%s: pos, energy, cell, pbc, climb and the state must be on one device" % who)
    check(lib().mdl_fire_step(ptr(pos), ptr(vel), ptr(force.contiguous()), ptr(fixed), ptr(state.band_node_ptr), N, B, ptr(fmax),
                              ptr(state.dt), ptr(state.alpha), ptr(state.n_pos), ptr(state.steps), ptr(state.done), ptr(state.fmax_seen),
                              int(c["n_min"]), float(c["f_inc"]), float(c["f_dec"]), float(c["alpha_start"]), float(c["f_alpha"]),
                              float(c["dt_max"]), float(c["maxstep"]), ptr(state.image_ptr), ptr(state.band_ptr), I,
                              ptr(energy.contiguous()), ptr(cell.contiguous()), ptr(pbc.contiguous()), ptr(spring), ptr(climb),
                              ptr(state.band_force), ptr(state.tangent_force), ptr(state.seg_len), ptr(state.climber), stream()),
          "mdl_fire_step")
    return state


# ------------------------------------------------------------------------------------------------
# Molecular dynamics: one BAOAB step of a batch of structures in one launch (csrc/md.hip)
# ------------------------------------------------------------------------------------------------
class MDState:
    """Per-structure state of md_step, [B] device tensors: steps (updates made) and status (0 running, 1 finished: steps reached
    n_steps and the last kick is closed, 2 refused: an atom would have moved further than max_disp, or to a non-finite place)
    int32; ekin float64, the kinetic energy at the positions the forces of the last call belong to."""

    __slots__ = ("steps", "status", "ekin", "_checked")

    def __init__(self, steps, status, ekin):
        self.steps, self.status, self.ekin = steps, status, ekin
        self._checked = {}                                     # operand -> the tensor whose values md_step has read back once

    def clone(self):
        new = MDState(self.steps.clone(), self.status.clone(), self.ekin.clone())
        new._checked = dict(self._checked)
        return new


def md_state(B, device=None):
    """A fresh MDState of B structures: no step made, every structure running."""
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    return MDState(torch.zeros(int(B), dtype=torch.int32, device=dev), torch.zeros(int(B), dtype=torch.int32, device=dev),
                   torch.zeros(int(B), dtype=torch.float64, device=dev))


# per-structure operand -> (dtype, its range: ">" above zero, ">=" not below, None any value)
_MD_PER_STRUCTURE = {"dt": (torch.float64, ">"), "gamma": (torch.float64, ">="), "kT": (torch.float64, ">="),
                     "n_steps": (torch.int32, ">="), "seed": (torch.int64, None), "pressure": (torch.float64, None),
                     "rate": (torch.float64, ">=")}


def _md_numbers(who, values):
    """the range of every operand given as a plain number — before a device or the library is asked for anything"""
    for name, v in values:
        rng = ">" if name in ("max_disp", "max_strain") else _MD_PER_STRUCTURE[name][1]
        if torch.is_tensor(v) or rng is None:
            continue
        if not (float(v) > 0.0 if rng == ">" else float(v) >= 0.0):           # (a NaN is neither)
            raise MdlError("%s: %s must be %s 0 (got %r)" % (who, name, rng, v))


def _md_in_range(who, name, t, rng, checked):
    """t > 0 (or >= 0) everywhere, read back ONCE per tensor: `checked` remembers which tensor, at which version, has passed"""
    seen, version = checked.get(name, (None, None))
    if rng is None or (seen is not None and seen() is t and version == t._version):
        return
    if not bool(((t > 0) if rng == ">" else (t >= 0)).all()):
        raise MdlError("%s: %s must be %s 0 everywhere" % (who, name, rng))
    checked[name] = (weakref.ref(t), t._version)


def _md_per_structure(who, values, B, dev, checked):
    """(name, a number or a [B] tensor) -> contiguous [B] device tensors of the operand's type; a plain seed s: s + b"""
    out = []
    for name, v in values:
        dtype, rng = _MD_PER_STRUCTURE[name]
        if torch.is_tensor(v):
            if v.dtype != dtype or tuple(v.shape) != (B,):
                raise MdlError("%s: %s must be a number or a [B] %s tensor with B = %d (got %s %s)" % (who, name, dtype, B, tuple(v.shape), v.dtype))
            require_hip(v)
            if v.device != dev:
                raise MdlError("%s: %s must be on the device of the other tensors" % (who, name))
            _md_in_range(who, name, v, rng, checked)
            out.append(v.contiguous())
        elif name == "seed":
            out.append(torch.arange(B, dtype=torch.int64, device=dev) + int(v))
        else:
            out.append(torch.full((B,), v, dtype=dtype, device=dev))
    return out


def _md_atoms(who, mass, node_ptr, fixed, checked):
    """the checks md_step and md_velocities share: mass [N] float64 > 0, node_ptr, fixed.  Returns (N, B, fixed as uint8 or None)"""
    require_hip(mass, node_ptr, fixed)
    if mass.dtype != torch.float64 or mass.dim() != 1 or not mass.is_contiguous():
        raise MdlError("%s: mass must be a contiguous [N] float64 tensor (got %s %s)" % (who, tuple(mass.shape), mass.dtype))
    N = mass.shape[0]
    if node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 1:
        raise MdlError("%s: node_ptr must be [B + 1] int64" % who)
    if fixed is not None:
        if fixed.dtype not in (torch.uint8, torch.bool) or tuple(fixed.shape) != (N,):
            raise MdlError("%s: fixed must be [N] uint8 or bool with N = %d (got %s %s)" % (who, N, tuple(fixed.shape), fixed.dtype))
        fixed = fixed.contiguous().view(torch.uint8)
    if any(t.device != mass.device for t in (node_ptr, fixed) if t is not None):
        raise MdlError("%s: mass, node_ptr and fixed must be on one device" % who)
    _md_in_range(who, "mass", mass, ">", checked)
    return N, node_ptr.numel() - 1, fixed


def md_step(pos, vel, force, mass, node_ptr, state, dt, n_steps, gamma=0.0, kT=0.0, seed=0, fixed=None, max_disp=0.5):
    """Everything between two force evaluations of a molecular-dynamics run, for every structure of a batch, in place, in ONE
    launch: BAOAB with one force evaluation per step (the kick that closes step n and B A O A of step n + 1 are one call).
      pos, vel [N, 3] float64 (updated in place: contiguous tensors), force [N, 3] float32 at pos, mass [N] float64 > 0, node_ptr
      [B + 1] int64, state an MDState of B structures (updated in place), fixed [N] uint8 / bool or None (non-zero: the atom stays
      where it is with zero velocity), max_disp > 0: a step that would move an atom further is refused as a whole (status 2,
      positions kept to the bit).
      Per structure, a number or a [B] tensor each: dt > 0 and gamma >= 0 (friction; 0: no thermostat, no random number), kT >= 0
      (float64), n_steps >= 0 (int32: the call at steps == n_steps closes the last kick and sets status 1), seed (int64; a plain
      integer s gives structure b the key s + b).
    Call it after EVERY evaluation, n_steps + 1 times in all; state.ekin is then the kinetic energy at the evaluated positions.
    The update, the counter layout of the noise (Philox4x32-10: a structure gets the same bits alone or in any batch) and the
    guard are stated in include/mdl_hip.h (mdl_md_step).  No atomics: two calls from the same inputs give the same bits.  No host
    synchronisation, except that the values of mass and of a tensor-valued dt, gamma, kT or n_steps are checked once per tensor (the
    state remembers which it has seen).  Returns state."""
    return _md_step("md_step", pos, vel, force, mass, node_ptr, state, dt, n_steps, gamma, kT, seed, fixed, max_disp)


def _md_step(who, pos, vel, force, mass, node_ptr, state, dt, n_steps, gamma, kT, seed, fixed, max_disp, baro=None):
    """md_step and md_cell_step (`who`) behind their arguments: the checks and the one launch.  baro: None, or md_cell_step's (cell,
    strain_grad, pressure, rate, max_strain): the cell mode of mdl_md_step."""
    state_type, maker = (MDState, "md_state") if baro is None else (MDCellState, "md_cell_state")
    if not isinstance(state, state_type):
        raise MdlError("%s: state must be an ops.%s (ops.%s)" % (who, state_type.__name__, maker))
    per = (("dt", dt), ("gamma", gamma), ("kT", kT), ("seed", seed), ("n_steps", n_steps))
    fields = (("steps", torch.int32), ("status", torch.int32), ("ekin", torch.float64))
    cell = strain_grad = None
    if baro is not None:
        cell, strain_grad, pressure, rate, max_strain = baro
        per += (("pressure", pressure), ("rate", rate))
        fields += (("volume", torch.float64), ("pressure", torch.float64))
    _md_numbers(who, per + (("max_disp", max_disp),) + ((("max_strain", max_strain),) if baro is not None else ()))
    if baro is not None:                                       # shapes that need no device to be wrong
        Bc = node_ptr.numel() - 1 if torch.is_tensor(node_ptr) else -1
        if not torch.is_tensor(cell) or cell.dtype != torch.float64 or tuple(cell.shape) != (Bc, 3, 3) or not cell.is_contiguous():
            raise MdlError("%s: cell must be a contiguous [B, 3, 3] float64 tensor with B = %d (got %s %s)"
                           % (who, Bc, tuple(getattr(cell, "shape", ())), getattr(cell, "dtype", type(cell))))
        if not torch.is_tensor(strain_grad) or strain_grad.dtype != torch.float32 or tuple(strain_grad.shape) != (Bc, 3, 3):
            raise MdlError("%s: strain_grad must be [B, 3, 3] float32 with B = %d (got %s %s)"
                           % (who, Bc, tuple(getattr(strain_grad, "shape", ())), getattr(strain_grad, "dtype", type(strain_grad))))
    state_tensors = [getattr(state, k) for k, _ in fields]
    require_hip(pos, vel, force, cell, strain_grad, *state_tensors)
    N, B, fixed = _md_atoms(who, mass, node_ptr, fixed, state._checked)
    for name, t in (("pos", pos), ("vel", vel)):
        if t.dtype != torch.float64 or tuple(t.shape) != (N, 3) or not t.is_contiguous():
            raise MdlError("%s: %s must be a contiguous [N, 3] float64 tensor with N = %d (got %s %s)" % (who, name, N, tuple(t.shape), t.dtype))
    if force.dtype != torch.float32 or tuple(force.shape) != (N, 3):
        raise MdlError("%s: force must be [N, 3] float32 with N = %d (got %s %s)" % (who, N, tuple(force.shape), force.dtype))
    for (k, dt_), t in zip(fields, state_tensors):
        if t.dtype != dt_ or tuple(t.shape) != (B,) or not t.is_contiguous():
            raise MdlError("%s: state.%s must be a contiguous [%d] %s tensor (got %s %s)" % (who, k, B, dt_, tuple(t.shape), t.dtype))
    if any(t.device != pos.device for t in [vel, force, mass] + state_tensors + ([] if baro is None else [cell, strain_grad])):
        raise MdlError("%s: pos, the other tensors and the state must be on one device" % who)
    per = _md_per_structure(who, per, B, pos.device, state._checked)
    dt, gamma, kT, seed, n_steps = per[:5]
    if baro is None:
        cell_args = [None] * 6 + [0.0]
    else:
        cell_args = [ptr(cell), ptr(strain_grad.contiguous()), ptr(per[5]), ptr(per[6]), ptr(state.volume), ptr(state.pressure), float(max_strain)]
    check(lib().mdl_md_step(ptr(pos), ptr(vel), ptr(force.contiguous()), ptr(mass), ptr(fixed), ptr(node_ptr.contiguous()), N, B, ptr(dt),
                            ptr(gamma), ptr(kT), ptr(seed), ptr(n_steps), ptr(state.steps), ptr(state.status), ptr(state.ekin),
                            float(max_disp), *cell_args, stream()), "mdl_md_step")
    return state


class MDCellState(MDState):
    """Per-structure state of md_cell_step: the MDState fields (status 3: refused by the strain guard — the barostat would have
    strained the cell by more than max_strain, or the cell has no volume) and what every call writes for a running structure:
    volume, |det cell|, and pressure, the instantaneous (2 ekin - tr dE/d eps) / (3 volume), [B] float64, at the positions the
    forces of the last call belong to; NaN where the cell has no volume."""

    __slots__ = ("volume", "pressure")

    def __init__(self, steps, status, ekin, volume, pressure):
        MDState.__init__(self, steps, status, ekin)
        self.volume, self.pressure = volume, pressure

    def clone(self):
        new = MDCellState(self.steps.clone(), self.status.clone(), self.ekin.clone(), self.volume.clone(), self.pressure.clone())
        new._checked = dict(self._checked)
        return new


def md_cell_state(B, device=None):
    """A fresh MDCellState of B structures: no step made, every structure running, volume and pressure not yet written (NaN)."""
    base = md_state(B, device)
    nan = lambda: torch.full((int(B),), float("nan"), dtype=torch.float64, device=base.ekin.device)
    return MDCellState(base.steps, base.status, base.ekin, nan(), nan())


def md_cell_step(pos, vel, cell, force, strain_grad, mass, node_ptr, state, dt, n_steps, pressure, rate, gamma=0.0, kT=0.0, seed=0, fixed=None,
                 max_disp=0.5, max_strain=0.03):
    """md_step at constant pressure: the same call with an isotropic barostat in it — stochastic cell rescaling (Bernetti & Bussi,
    J. Chem. Phys. 153, 114107 (2020)) in eps = ln V —, for every structure of a batch, in place, still in ONE launch.
      pos, vel, force, mass, node_ptr, dt, n_steps, gamma, kT, seed, fixed, max_disp   as md_step
      cell [B, 3, 3] float64 (rows are lattice vectors; updated in place: a contiguous tensor), strain_grad [B, 3, 3] float32 (dE/d eps,
      NOT divided by the volume: ForceField.evaluate(stress=True, volume_normalised=False)), state an MDCellState (ops.md_cell_state;
      updated in place: volume and pressure are written for every running structure)
      Per structure, a number or a [B] float64 tensor each: pressure (the target, any sign; in the energy unit per volume) and
      rate >= 0 (compressibility / tau_p; 0: no barostat — the structure gets the bits of md_step and its cell is not written)
      max_strain > 0: a step whose volume strain |d eps| would exceed it is refused as a whole (status 3, positions and cell kept to
      the bit); the default 0.03 is a 1 % linear change per step.  max_disp then bounds the thermal motion alone.
    With kT == 0 the barostat draws no number (the Berendsen limit).  The forces are those of the unscaled positions: first-order
    splitting.  The update, the counter of the barostat's noise (tag 2) and the guards are stated in include/mdl_hip.h (mdl_md_step,
    the cell mode).  No atomics, no host synchronisation beyond md_step's (a tensor-valued rate is checked once).  Returns state."""
    return _md_step("md_cell_step", pos, vel, force, mass, node_ptr, state, dt, n_steps, gamma, kT, seed, fixed, max_disp,
                    (cell, strain_grad, pressure, rate, max_strain))


def md_velocities(mass, node_ptr, kT, seed=0, fixed=None, zero_momentum=True):
    """Maxwell-Boltzmann velocities [N, 3] float64 for mass [N] float64 > 0 at kT >= 0 (a number or a [B] float64 tensor): v_i =
    sqrt(kT / m_i) xi_i from the noise of md_step (tag 1, step word 0; seed as there), fixed atoms 0.  zero_momentum: the momentum
    of the free atoms of every structure with at least two of them is removed (the temperature of that draw is then kT (n - 1) / n
    on average).  One launch, the same bits from the same seed whatever else is in the batch; rows outside every structure are 0."""
    who = "md_velocities"
    per = (("kT", kT), ("seed", seed))
    _md_numbers(who, per)
    checked = {}
    N, B, fixed = _md_atoms(who, mass, node_ptr, fixed, checked)
    kT, seed = _md_per_structure(who, per, B, mass.device, checked)
    vel = torch.zeros((N, 3), dtype=torch.float64, device=mass.device)
    check(lib().mdl_md_velocities(ptr(vel), ptr(mass), ptr(fixed), ptr(node_ptr.contiguous()), N, B, ptr(kT), ptr(seed),
                                  1 if zero_momentum else 0, stream()), "mdl_md_velocities")
    return vel


# ------------------------------------------------------------------------------------------------
# Trajectory observables: pair histograms and mean-squared displacements of a batch, one launch per sampled frame each
# (csrc/observe.hip, include/mdl_hip_analysis.h)
# ------------------------------------------------------------------------------------------------
# the limits of include/mdl_hip_analysis.h, restated here so that a request beyond them is refused before the library is loaded
RDF_MAX_COUNTERS, RDF_MAX_IMAGES, MSD_MAX_TYPES = 8192, 16, 64
RDF_NO_VOLUME, RDF_TOO_MANY_IMAGES, RDF_BAD_TYPE, RDF_TOO_LARGE = 1, 2, 4, 8


def observe_numbers(who, n_types=None, rdf=None, msd=None):
    """The ranges of what an observation is asked with — plain numbers, checked before a device or the library is asked for
    anything.  rdf: None or dict(r_max, nbins); msd: None or dict(n_lags, origin_every[, n_origins, remove_com]).  Returns (rdf, msd)
    as dicts with every key present (n_origins defaults to ceil(n_lags / origin_every): an origin lives until its lag is n_lags)."""
    if n_types is not None and int(n_types) < 1:
        raise MdlError("%s: the number of types must be >= 1 (got %r)" % (who, n_types))
    if rdf is not None:
        unknown = set(rdf) - {"r_max", "nbins"}
        if unknown or "r_max" not in rdf or "nbins" not in rdf:
            raise MdlError("%s: rdf must be dict(r_max, nbins) (got keys %s)" % (who, sorted(rdf)))
        r_max, nbins = float(rdf["r_max"]), int(rdf["nbins"])
        if not (r_max > 0.0 and r_max < float("inf")):
            raise MdlError("%s: rdf: r_max must be > 0 and finite (got %r)" % (who, rdf["r_max"]))
        if nbins < 1:
            raise MdlError("%s: rdf: nbins must be >= 1 (got %r)" % (who, rdf["nbins"]))
        if n_types is not None and int(n_types) * (int(n_types) + 1) // 2 * nbins > RDF_MAX_COUNTERS:
            raise MdlError("%s: rdf: T (T + 1) / 2 * nbins = %d counters with T = %d types exceed the %d of the kernel's LDS histogram"
                           % (who, int(n_types) * (int(n_types) + 1) // 2 * nbins, int(n_types), RDF_MAX_COUNTERS))
        rdf = dict(r_max=r_max, nbins=nbins)
    if msd is not None:
        unknown = set(msd) - {"n_lags", "origin_every", "n_origins", "remove_com"}
        if unknown or "n_lags" not in msd:
            raise MdlError("%s: msd must be dict(n_lags, origin_every[, n_origins, remove_com]) (got keys %s)" % (who, sorted(msd)))
        n_lags, origin_every = int(msd["n_lags"]), int(msd.get("origin_every", 1))
        if n_lags < 1:
            raise MdlError("%s: msd: n_lags must be >= 1 (got %r)" % (who, msd["n_lags"]))
        if origin_every < 1:
            raise MdlError("%s: msd: origin_every must be >= 1 (got %r)" % (who, msd["origin_every"]))
        n_origins = msd.get("n_origins")
        n_origins = -(-n_lags // origin_every) if n_origins is None else int(n_origins)
        if not 1 <= n_origins <= 65535:
            raise MdlError("%s: msd: n_origins must be in 1 .. 65535 (got %r)" % (who, n_origins))
        if n_types is not None and int(n_types) > MSD_MAX_TYPES:
            raise MdlError("%s: msd: at most %d types (got %d)" % (who, MSD_MAX_TYPES, int(n_types)))
        msd = dict(n_lags=n_lags, origin_every=origin_every, n_origins=n_origins, remove_com=bool(msd.get("remove_com", True)))
    return rdf, msd


def msd_schedule(n_samples, n_lags, origin_every, n_origins):
    """The ring of time origins as host arithmetic, for samples s = 0 .. n_samples - 1: (slot [n_samples] — the slot that takes the
    positions of sample s as a new origin BEFORE the sample is accumulated, every origin_every samples into (s // origin_every) %
    n_origins, else -1 —, lag [n_samples, n_origins] int32 — how many samples ago the origin of every slot was stored, -1 where the
    slot is empty or its lag has reached n_lags).  Live slots of a sample have distinct lags; lag 0 is the origin just stored."""
    n_samples, n_lags, origin_every, n_origins = int(n_samples), int(n_lags), int(origin_every), int(n_origins)
    slot = torch.full((n_samples,), -1, dtype=torch.int64)
    lag = torch.full((n_samples, n_origins), -1, dtype=torch.int32)
    stored = [-1] * n_origins
    for s in range(n_samples):
        if s % origin_every == 0:
            slot[s] = (s // origin_every) % n_origins
            stored[int(slot[s])] = s
        for k, s0 in enumerate(stored):
            if s0 >= 0 and s - s0 < n_lags:
                lag[s, k] = s - s0
    return slot, lag


class ObserveState:
    """The accumulators of rdf_accumulate and msd_accumulate, device tensors allocated once (ops.observe_state):
      types [N] int32, node_ptr [B + 1] int64, n_types T, max_atoms (the largest structure: it sizes the histogram's grid)
      rdf: r_max, nbins; hist [B, T (T + 1) / 2, nbins] int64 — the unordered pair (a <= b) at pair_index(a, b) —, frames [B] int64,
           vol_sum [B] float64, flag [B] int32 (bits RDF_NO_VOLUME, RDF_TOO_MANY_IMAGES, RDF_BAD_TYPE, RDF_TOO_LARGE)
      msd: n_lags, origins [K, N, 3] float64 (the ring; the caller stores an origin with origins[k].copy_(pos)), msd_sum [B, T, n_lags]
           float64, msd_count [B, n_lags] int64
    What was not asked for is None."""

    __slots__ = ("types", "node_ptr", "n_types", "max_atoms", "r_max", "nbins", "hist", "frames", "vol_sum", "flag", "n_lags", "origins",
                 "msd_sum", "msd_count")

    def pair_index(self, a, b):
        a, b = (int(a), int(b)) if int(a) <= int(b) else (int(b), int(a))
        if not 0 <= a <= b < self.n_types:
            raise MdlError("pair_index: types must be in 0 .. %d (got %d, %d)" % (self.n_types - 1, a, b))
        return a * self.n_types - a * (a - 1) // 2 + (b - a)


def _host_ints(who, name, v):
    t = v.detach().cpu() if torch.is_tensor(v) else torch.as_tensor(v)
    if t.dtype in (torch.float16, torch.float32, torch.float64, torch.bfloat16, torch.bool) or t.dim() != 1:
        raise MdlError("%s: %s must be a one-dimensional integer array (got %s %s)" % (who, name, tuple(t.shape), t.dtype))
    return t.to(torch.int64)


def _state_atoms(who, types, node_ptr, n_types):
    """what observe_state and vacf_state look at once on the host: (types, node_ptr as int64 host tensors, N, B, T)"""
    th, ph = _host_ints(who, "types", types), _host_ints(who, "node_ptr", node_ptr)
    N, B = th.numel(), ph.numel() - 1
    if B < 0 or (B >= 0 and (int(ph[0]) != 0 or int(ph[-1]) != N or bool((ph[1:] < ph[:-1]).any()))):
        raise MdlError("%s: node_ptr must start at 0, be non-decreasing and end at N = %d" % (who, N))
    T = int(n_types) if n_types is not None else (int(th.max()) + 1 if N else 1)
    if N and (int(th.min()) < 0 or int(th.max()) >= T):
        raise MdlError("%s: types must be in 0 .. %d (got %d .. %d)" % (who, T - 1, int(th.min()), int(th.max())))
    return th, ph, N, B, T


def observe_state(types, node_ptr, n_types=None, rdf=None, msd=None, device=None):
    """A fresh ObserveState.  types [N] integers in 0 .. n_types - 1 (n_types None: the largest type + 1) and node_ptr [B + 1], arrays
    or tensors: their values are looked at here, once — a device tensor is read back — so that no launch sees a type it cannot
    index or a structure larger than its grid.  rdf: None or dict(r_max, nbins) with T (T + 1) / 2 * nbins <= RDF_MAX_COUNTERS; msd:
    None or dict(n_lags[, origin_every, n_origins]) (the state keeps n_lags and a ring of n_origins slots; the schedule is the
    caller's: ops.msd_schedule).  Every argument error raises before a device or the library is asked for anything."""
    who = "observe_state"
    observe_numbers(who, n_types, rdf, msd)
    th, ph, N, B, T = _state_atoms(who, types, node_ptr, n_types)
    rdf, msd = observe_numbers(who, T, rdf, msd)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    st = ObserveState()
    for k in ObserveState.__slots__:
        setattr(st, k, None)
    st.types = (types.detach().to(dev, torch.int32) if torch.is_tensor(types) else th.to(torch.int32).to(dev)).contiguous()
    st.node_ptr = (node_ptr.detach().to(dev, torch.int64) if torch.is_tensor(node_ptr) else ph.to(dev)).contiguous()
    st.n_types, st.max_atoms = T, int((ph[1:] - ph[:-1]).max()) if B > 0 else 0
    z = lambda shape, dtype: torch.zeros(shape, dtype=dtype, device=dev)
    if rdf is not None:
        st.r_max, st.nbins = rdf["r_max"], rdf["nbins"]
        st.hist, st.frames = z((B, T * (T + 1) // 2, st.nbins), torch.int64), z((B,), torch.int64)
        st.vol_sum, st.flag = z((B,), torch.float64), z((B,), torch.int32)
    if msd is not None:
        st.n_lags = msd["n_lags"]
        st.origins = z((msd["n_origins"], N, 3), torch.float64)
        st.msd_sum, st.msd_count = z((B, T, st.n_lags), torch.float64), z((B, st.n_lags), torch.int64)
    return st


def _observe_common(who, pos, state, status, asked):
    if not isinstance(state, ObserveState) or getattr(state, asked) is None:
        raise MdlError("%s: state must be an ops.ObserveState made for it (ops.observe_state)" % who)
    if not torch.is_tensor(pos) or pos.dtype != torch.float64 or pos.dim() != 2 or pos.shape[1] != 3 or not pos.is_contiguous():
        raise MdlError("%s: pos must be a contiguous [N, 3] float64 tensor (got %s %s)"
                       % (who, tuple(getattr(pos, "shape", ())), getattr(pos, "dtype", type(pos))))
    N, B = state.types.numel(), state.node_ptr.numel() - 1
    if pos.shape[0] != N:
        raise MdlError("%s: pos must be [N, 3] with N = %d, the atoms of the state (got %s)" % (who, N, tuple(pos.shape)))
    if status is not None and (not torch.is_tensor(status) or status.dtype != torch.int32 or tuple(status.shape) != (B,)
                               or not status.is_contiguous()):
        raise MdlError("%s: status must be a contiguous [B] int32 tensor with B = %d, or None" % (who, B))
    return N, B


def rdf_accumulate(pos, cell, pbc, state, status=None):
    """One frame into the pair histograms of a batch: ONE launch, no host read (include/mdl_hip_analysis.h, mdl_rdf_accumulate).
      pos [N, 3] float64, unwrapped; cell [B, 3, 3] float64, rows are lattice vectors; pbc [B] int32, one bit per periodic axis;
      state an ObserveState made with rdf=dict(r_max, nbins) (its types and node_ptr are used); status [B] int32 or None: structures
      with a non-zero status are skipped (ops.md_step sets it where its guard stopped a structure).
    For every structure every ordered pair (i, j, image) with 0 < r < r_max — every periodic image, whatever the skew of the cell
    and however far the unwrapped atoms have drifted — is counted in state.hist[b, pair, (int)(r nbins / r_max)]; state.frames[b] += 1
    and state.vol_sum[b] += |det cell|.  A structure whose periodic axes span no volume, or that needs more than RDF_MAX_IMAGES
    images along an axis, is not counted and gets a bit in state.flag.  Integer counts: the same bits on every run and in any
    batch.  Returns state."""
    who = "rdf_accumulate"
    N, B = _observe_common(who, pos, state, status, "hist")
    if not torch.is_tensor(cell) or cell.dtype != torch.float64 or tuple(cell.shape) != (B, 3, 3) or not cell.is_contiguous():
        raise MdlError("%s: cell must be a contiguous [B, 3, 3] float64 tensor with B = %d" % (who, B))
    if not torch.is_tensor(pbc) or pbc.dtype != torch.int32 or tuple(pbc.shape) != (B,) or not pbc.is_contiguous():
        raise MdlError("%s: pbc must be a contiguous [B] int32 tensor (one bit per axis) with B = %d" % (who, B))
    require_hip(pos, cell, pbc, status, state.hist)
    if any(t.device != pos.device for t in (cell, pbc, state.hist) + (() if status is None else (status,))):
        raise MdlError("%s: pos, cell, pbc, status and the state must be on one device" % who)
    check(lib().mdl_rdf_accumulate(ptr(pos), ptr(state.types), ptr(state.node_ptr), ptr(cell), ptr(pbc), ptr(status), N, B, state.max_atoms,
                                   float(state.r_max), int(state.nbins), int(state.n_types), ptr(state.hist), ptr(state.frames),
                                   ptr(state.vol_sum), ptr(state.flag), stream()), "mdl_rdf_accumulate")
    return state


def msd_accumulate(pos, lag, mass, state, fixed=None, status=None, remove_com=True):
    """One frame into the mean-squared displacements of a batch against the ring of origins state.origins: ONE launch, no host read
    (include/mdl_hip_analysis.h, mdl_msd_accumulate).
      pos [N, 3] float64; lag [K] int32 ON THE DEVICE, one per slot of the ring: how many samples ago state.origins[k] was stored,
      negative: skip the slot (a row of ops.msd_schedule's table; live slots must have distinct lags); mass [N] float64; state an
      ObserveState made with msd=...; fixed [N] uint8 / bool or None (fixed atoms are left out); status as rdf_accumulate.
    state.msd_sum[b, t, lag[k]] += the sum over the free atoms of type t of |x - x0 - D|^2, D the displacement of the free atoms'
    centre of mass since that origin (remove_com) or 0; state.msd_count[b, lag[k]] += 1.  No atomics: the same bits on every run,
    alone and in any batch.  Returns state."""
    who = "msd_accumulate"
    N, B = _observe_common(who, pos, state, status, "msd_sum")
    K = state.origins.shape[0]
    if not torch.is_tensor(lag) or lag.dtype != torch.int32 or tuple(lag.shape) != (K,) or not lag.is_contiguous():
        raise MdlError("%s: lag must be a contiguous [K] int32 tensor with K = %d, the slots of state.origins" % (who, K))
    if not torch.is_tensor(mass) or mass.dtype != torch.float64 or tuple(mass.shape) != (N,) or not mass.is_contiguous():
        raise MdlError("%s: mass must be a contiguous [N] float64 tensor with N = %d" % (who, N))
    if fixed is not None:
        if not torch.is_tensor(fixed) or fixed.dtype not in (torch.uint8, torch.bool) or tuple(fixed.shape) != (N,):
            raise MdlError("%s: fixed must be [N] uint8 or bool with N = %d, or None" % (who, N))
        fixed = fixed.contiguous().view(torch.uint8)
    require_hip(pos, lag, mass, fixed, status, state.msd_sum)
    if any(t.device != pos.device for t in (lag, mass, state.msd_sum) + tuple(t for t in (fixed, status) if t is not None)):
        raise MdlError("%s: pos, lag, mass, fixed, status and the state must be on one device" % who)
    check(lib().mdl_msd_accumulate(ptr(pos), ptr(state.origins), ptr(lag), ptr(mass), ptr(state.types), ptr(fixed), ptr(state.node_ptr),
                                   ptr(status), N, B, K, int(state.n_types), int(state.n_lags), 1 if remove_com else 0, ptr(state.msd_sum),
                                   ptr(state.msd_count), stream()), "mdl_msd_accumulate")
    return state


# ------------------------------------------------------------------------------------------------
# Time correlations: the on-step velocity and the velocity autocorrelation of a batch, one launch each
# (csrc/vacf.hip, include/mdl_hip_dynamics.h)
# ------------------------------------------------------------------------------------------------
def md_onstep_velocity(vel, force, mass, node_ptr, state, dt, fixed=None, out=None):
    """The velocity AT the positions `force` was evaluated at, [N, 3] float64, in ONE launch and without a host read
    (include/mdl_hip_dynamics.h, mdl_md_onstep_velocity).  Between two calls of md_step `vel` lacks the closing half kick of the step;
    md_step applies it at the start of its next call.  Called between an evaluation and that call, this restates the kick on the same
    operands: v = fma(dt / 2, (double) force / mass, vel) where state.steps > 0, v = vel where no step has been made, 0 for a fixed atom
    — bit for bit the velocity whose kinetic energy the next md_step writes to state.ekin, and what its closing call stores.
      vel [N, 3] float64 and force [N, 3] float32 (contiguous), mass [N] float64, node_ptr [B + 1] int64, state an MDState or an
      MDCellState (its steps and status are read, nothing is written; under md_cell_step the result is the velocity BEFORE the
      barostat's 1 / s scaling of that step), dt a number or a [B] float64 tensor, fixed [N] uint8 / bool or None, out [N, 3] float64
      (contiguous) or None for a new tensor of zeros.
    The rows of a structure with a non-zero status, or outside every structure, are not written.  Returns out."""
    who = "md_onstep_velocity"
    if not isinstance(state, MDState):
        raise MdlError("%s: state must be an ops.MDState or ops.MDCellState (ops.md_state, ops.md_cell_state)" % who)
    if not torch.is_tensor(vel) or vel.dtype != torch.float64 or vel.dim() != 2 or vel.shape[1] != 3 or not vel.is_contiguous():
        raise MdlError("%s: vel must be a contiguous [N, 3] float64 tensor (got %s %s)"
                       % (who, tuple(getattr(vel, "shape", ())), getattr(vel, "dtype", type(vel))))
    N = vel.shape[0]
    if not torch.is_tensor(force) or force.dtype != torch.float32 or tuple(force.shape) != (N, 3) or not force.is_contiguous():
        raise MdlError("%s: force must be a contiguous [N, 3] float32 tensor with N = %d (got %s %s)"
                       % (who, N, tuple(getattr(force, "shape", ())), getattr(force, "dtype", type(force))))
    if not torch.is_tensor(mass) or mass.dtype != torch.float64 or tuple(mass.shape) != (N,) or not mass.is_contiguous():
        raise MdlError("%s: mass must be a contiguous [N] float64 tensor with N = %d" % (who, N))
    if not torch.is_tensor(node_ptr) or node_ptr.dtype != torch.int64 or node_ptr.dim() != 1 or node_ptr.numel() < 1 or not node_ptr.is_contiguous():
        raise MdlError("%s: node_ptr must be a contiguous [B + 1] int64 tensor" % who)
    B = node_ptr.numel() - 1
    for k in ("steps", "status"):
        t = getattr(state, k)
        if t.dtype != torch.int32 or tuple(t.shape) != (B,) or not t.is_contiguous():
            raise MdlError("%s: state.%s must be a contiguous [%d] int32 tensor (got %s %s)" % (who, k, B, tuple(t.shape), t.dtype))
    if torch.is_tensor(dt):
        if dt.dtype != torch.float64 or tuple(dt.shape) != (B,) or not dt.is_contiguous():
            raise MdlError("%s: dt must be a number or a contiguous [B] float64 tensor with B = %d (got %s %s)" % (who, B, tuple(dt.shape), dt.dtype))
    elif not float(dt) > 0.0:                                  # (a NaN is not)
        raise MdlError("%s: dt must be > 0 (got %r)" % (who, dt))
    if fixed is not None:
        if not torch.is_tensor(fixed) or fixed.dtype not in (torch.uint8, torch.bool) or tuple(fixed.shape) != (N,):
            raise MdlError("%s: fixed must be [N] uint8 or bool with N = %d, or None" % (who, N))
        fixed = fixed.contiguous().view(torch.uint8)
    if out is not None and (not torch.is_tensor(out) or out.dtype != torch.float64 or tuple(out.shape) != (N, 3) or not out.is_contiguous()):
        raise MdlError("%s: out must be a contiguous [N, 3] float64 tensor with N = %d, or None" % (who, N))
    tensors = [force, mass, node_ptr, state.steps, state.status] + [t for t in (dt if torch.is_tensor(dt) else None, fixed, out) if t is not None]
    require_hip(vel, *tensors)
    if any(t.device != vel.device for t in tensors):
        raise MdlError("%s: vel, the other tensors and the state must be on one device" % who)
    if not torch.is_tensor(dt):
        dt = torch.full((B,), float(dt), dtype=torch.float64, device=vel.device)
    if out is None:
        out = torch.zeros((N, 3), dtype=torch.float64, device=vel.device)
    check(lib().mdl_md_onstep_velocity(ptr(vel), ptr(force), ptr(mass), ptr(fixed), ptr(node_ptr), ptr(dt), ptr(state.steps), ptr(state.status),
                                       N, B, ptr(out), stream()), "mdl_md_onstep_velocity")
    return out


def vacf_numbers(who, n_types=None, vacf=None):
    """The ranges of what a velocity autocorrelation is asked with: dict(n_lags[, origin_every, n_origins, remove_com]), the ranges and
    defaults of observe_numbers' msd.  Plain numbers, checked before a device or the library is asked for anything.  Returns the dict
    with every key present, or None."""
    try:
        return observe_numbers(who, n_types, None, vacf)[1]
    except MdlError as e:
        raise MdlError(str(e).replace("msd", "vacf")) from None


class VacfState:
    """The accumulators of vacf_accumulate, device tensors allocated once (ops.vacf_state):
      types [N] int32, node_ptr [B + 1] int64, n_types T, n_lags, origins [K, N, 3] float64 (the ring; the caller stores an origin with
      origins[k].copy_(v)), vacf_sum [B, 2, T, n_lags] float64 (plane 0: the sum of u . u0 per type, plane 1: of m u . u0), vacf_count
      [B, n_lags] int64."""

    __slots__ = ("types", "node_ptr", "n_types", "n_lags", "origins", "vacf_sum", "vacf_count")


def vacf_state(types, node_ptr, n_types=None, vacf=None, device=None):
    """A fresh VacfState.  types [N] integers in 0 .. n_types - 1 (n_types None: the largest type + 1) and node_ptr [B + 1], arrays or
    tensors, looked at here once as in observe_state; vacf: dict(n_lags[, origin_every, n_origins]) (the state keeps n_lags and a ring of
    n_origins slots; the schedule is the caller's: ops.msd_schedule).  Every argument error raises before a device or the library is
    asked for anything."""
    who = "vacf_state"
    if vacf is None:
        raise MdlError("%s: vacf must be dict(n_lags[, origin_every, n_origins, remove_com])" % who)
    vacf_numbers(who, n_types, vacf)
    th, ph, N, B, T = _state_atoms(who, types, node_ptr, n_types)
    vacf = vacf_numbers(who, T, vacf)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    st = VacfState()
    st.types = (types.detach().to(dev, torch.int32) if torch.is_tensor(types) else th.to(torch.int32).to(dev)).contiguous()
    st.node_ptr = (node_ptr.detach().to(dev, torch.int64) if torch.is_tensor(node_ptr) else ph.to(dev)).contiguous()
    st.n_types, st.n_lags = T, vacf["n_lags"]
    st.origins = torch.zeros((vacf["n_origins"], N, 3), dtype=torch.float64, device=dev)
    st.vacf_sum = torch.zeros((B, 2, T, st.n_lags), dtype=torch.float64, device=dev)
    st.vacf_count = torch.zeros((B, st.n_lags), dtype=torch.int64, device=dev)
    return st


def vacf_accumulate(v, lag, mass, state, fixed=None, status=None, remove_com=True):
    """One frame into the velocity autocorrelation of a batch against the ring of origins state.origins: ONE launch, no host read
    (include/mdl_hip_dynamics.h, mdl_vacf_accumulate).
      v [N, 3] float64, the ON-STEP velocities (ops.md_onstep_velocity); lag [K] int32 ON THE DEVICE, one per slot of the ring: how
      many samples ago state.origins[k] was stored, negative: skip the slot (a row of ops.msd_schedule's table; live slots must have
      distinct lags); mass [N] float64; state a VacfState; fixed [N] uint8 / bool or None (fixed atoms are left out); status [B] int32
      or None: structures with a non-zero status are skipped.
    With u = v - U and u0 = v0 - U0, U and U0 the velocity of the centre of mass of the structure's free atoms now and at the origin
    (remove_com) or 0: state.vacf_sum[b, 0, t, lag[k]] += the sum over the free atoms of type t of u . u0, state.vacf_sum[b, 1, t,
    lag[k]] += that of m u . u0, state.vacf_count[b, lag[k]] += 1.  No atomics: the same bits on every run, alone and in any batch.
    Returns state."""
    who = "vacf_accumulate"
    if not isinstance(state, VacfState):
        raise MdlError("%s: state must be an ops.VacfState (ops.vacf_state)" % who)
    if not torch.is_tensor(v) or v.dtype != torch.float64 or v.dim() != 2 or v.shape[1] != 3 or not v.is_contiguous():
        raise MdlError("%s: v must be a contiguous [N, 3] float64 tensor (got %s %s)"
                       % (who, tuple(getattr(v, "shape", ())), getattr(v, "dtype", type(v))))
    N, B, K = state.types.numel(), state.node_ptr.numel() - 1, state.origins.shape[0]
    if v.shape[0] != N:
        raise MdlError("%s: v must be [N, 3] with N = %d, the atoms of the state (got %s)" % (who, N, tuple(v.shape)))
    if status is not None and (not torch.is_tensor(status) or status.dtype != torch.int32 or tuple(status.shape) != (B,)
                               or not status.is_contiguous()):
        raise MdlError("%s: status must be a contiguous [B] int32 tensor with B = %d, or None" % (who, B))
    if not torch.is_tensor(lag) or lag.dtype != torch.int32 or tuple(lag.shape) != (K,) or not lag.is_contiguous():
        raise MdlError("%s: lag must be a contiguous [K] int32 tensor with K = %d, the slots of state.origins" % (who, K))
    if not torch.is_tensor(mass) or mass.dtype != torch.float64 or tuple(mass.shape) != (N,) or not mass.is_contiguous():
        raise MdlError("%s: mass must be a contiguous [N] float64 tensor with N = %d" % (who, N))
    if fixed is not None:
        if not torch.is_tensor(fixed) or fixed.dtype not in (torch.uint8, torch.bool) or tuple(fixed.shape) != (N,):
            raise MdlError("%s: fixed must be [N] uint8 or bool with N = %d, or None" % (who, N))
        fixed = fixed.contiguous().view(torch.uint8)
    require_hip(v, lag, mass, fixed, status, state.vacf_sum)
    if any(t.device != v.device for t in (lag, mass, state.vacf_sum) + tuple(t for t in (fixed, status) if t is not None)):
        raise MdlError("%s: v, lag, mass, fixed, status and the state must be on one device" % who)
    check(lib().mdl_vacf_accumulate(ptr(v), ptr(state.origins), ptr(lag), ptr(mass), ptr(state.types), ptr(fixed), ptr(state.node_ptr),
                                    ptr(status), N, B, K, int(state.n_types), int(state.n_lags), 1 if remove_com else 0, ptr(state.vacf_sum),
                                    ptr(state.vacf_count), stream()), "mdl_vacf_accumulate")
    return state


# ------------------------------------------------------------------------------------------------
# Reciprocal space: the density modes of a batch at a list of reciprocal-lattice vectors and the partial structure factors /
# intermediate scattering functions formed from them, one launch each per sampled frame
# (csrc/sq.hip, include/mdl_hip_scattering.h)
# ------------------------------------------------------------------------------------------------
# the limits and flag bits of include/mdl_hip_scattering.h, restated here so that a request beyond them is refused before the
# library is loaded
SQ_MAX_TYPES = 8
SQ_NOT_PERIODIC, SQ_NO_VOLUME, SQ_BAD_TYPE, SQ_FATAL = 1, 2, 4, 3
SQ_MAX_Q = 65535 * 256
SQ_MAX_BYTES = 2 ** 30


def sq_half_space(n_max):
    """[Q, 3] int32: every non-zero integer triple n with max |n_k| <= n_max whose first non-zero component is positive — n and -n
    carry the same information —, in lexicographic order; Q = ((2 n_max + 1)^3 - 1) / 2"""
    n_max = int(n_max)
    r = range(-n_max, n_max + 1)
    return np.array([(i, j, k) for i in r for j in r for k in r if (i, j, k) > (0, 0, 0)], np.int32).reshape(-1, 3)


def _pair_index(a, b, T):
    a, b = (int(a), int(b)) if int(a) <= int(b) else (int(b), int(a))
    if not 0 <= a <= b < T:
        raise MdlError("pair_index: types must be in 0 .. %d (got %d, %d)" % (T - 1, a, b))
    return a * T - a * (a - 1) // 2 + (b - a)


def sq_numbers(who, n_types=None, sq=None, n_structs=None):
    """The ranges of what a structure-factor request is asked with — plain numbers, checked before a device or the library is asked
    for anything.  sq: None, or dict(q=<[Q, 3] integer array> | n_max=<int >= 1>[, fqt=None | dict(n_lags, origin_every[, n_origins]),
    max_bytes=2^30]).  With n_types and n_structs (B) known, the bytes of the two large buffers, f_sum and the ring of origins,
    8 B P n_lags Q + 16 K B T Q with P = T (T + 1) / 2, are held against max_bytes.  Returns dict(q, fqt, max_bytes) — q a
    [Q, 3] int32 numpy array (n_max written out), fqt None or dict(n_lags, origin_every, n_origins): a request itself —, or None."""
    if n_types is not None and int(n_types) < 1:
        raise MdlError("%s: the number of types must be >= 1 (got %r)" % (who, n_types))
    if sq is None:
        return None
    form = "dict(q=[Q, 3] integers | n_max=int >= 1[, fqt=dict(n_lags, origin_every[, n_origins]), max_bytes])"
    if not isinstance(sq, dict) or set(sq) - {"q", "n_max", "fqt", "max_bytes"} or (sq.get("q") is None) == (sq.get("n_max") is None):
        raise MdlError("%s: sq must be %s, with exactly one of q and n_max (got %s)"
                       % (who, form, sorted(sq) if isinstance(sq, dict) else type(sq).__name__))
    if sq.get("n_max") is not None:
        n_max = sq["n_max"]
        if isinstance(n_max, bool) or not isinstance(n_max, (int, np.integer)) or n_max < 1:
            raise MdlError("%s: sq: n_max must be an integer >= 1 (got %r)" % (who, n_max))
        n_max = int(n_max)
        if ((2 * n_max + 1) ** 3 - 1) // 2 > SQ_MAX_Q:
            raise MdlError("%s: sq: n_max = %d gives more than %d vectors" % (who, n_max, SQ_MAX_Q))
        q = sq_half_space(n_max)
    else:
        q = sq["q"]
        q = np.asarray(q.detach().cpu() if torch.is_tensor(q) else q)
        if q.ndim != 2 or q.shape[1] != 3 or q.dtype.kind not in "iu":
            raise MdlError("%s: sq: q must be a [Q, 3] integer array (got %s %s)" % (who, q.shape, q.dtype))
        if q.size and int(np.abs(q.astype(np.int64)).max()) >= 2 ** 31:
            raise MdlError("%s: sq: the components of q must fit 32 bits" % who)
        if q.shape[0] > SQ_MAX_Q:
            raise MdlError("%s: sq: at most %d vectors (got %d)" % (who, SQ_MAX_Q, q.shape[0]))
        q = np.ascontiguousarray(q.astype(np.int32))
    if n_types is not None and int(n_types) > SQ_MAX_TYPES:
        raise MdlError("%s: sq: at most %d types (got %d)" % (who, SQ_MAX_TYPES, int(n_types)))
    fqt = sq.get("fqt")
    if fqt is not None:
        if not isinstance(fqt, dict) or "remove_com" in fqt:
            raise MdlError("%s: sq: fqt must be dict(n_lags, origin_every[, n_origins]) (got %r)" % (who, fqt))
        try:
            fqt = observe_numbers(who, None, None, fqt)[1]
        except MdlError as e:
            raise MdlError(str(e).replace("msd: ", "sq: fqt: ").replace("msd must be dict(n_lags, origin_every[, n_origins, remove_com])",
                                                                      "sq: fqt must be dict(n_lags, origin_every[, n_origins])")) from None
        del fqt["remove_com"]
    max_bytes = sq.get("max_bytes")
    max_bytes = SQ_MAX_BYTES if max_bytes is None else int(max_bytes)
    if max_bytes < 0:
        raise MdlError("%s: sq: max_bytes must be >= 0 (got %r)" % (who, sq["max_bytes"]))
    if n_types is not None and n_structs is not None and fqt is not None:
        B, T, Q, K, n_lags = int(n_structs), int(n_types), q.shape[0], fqt["n_origins"], fqt["n_lags"]
        P = T * (T + 1) // 2
        need = 8 * B * P * n_lags * Q + 16 * K * B * T * Q
        if need > max_bytes:
            raise MdlError("%s: sq: fqt needs 8·B·P·n_lags·Q + 16·K·B·T·Q = %d bytes for f_sum and the ring of origins (B = %d structures, "
                           "T = %d types, P = %d pairs, Q = %d vectors, n_lags = %d, K = %d origins), more than max_bytes = %d"
                           % (who, need, B, T, P, Q, n_lags, K, max_bytes))
    return dict(q=q, fqt=fqt, max_bytes=max_bytes)


class SqState:
    """The buffers of density_modes and sq_accumulate, device tensors allocated once (ops.sq_state):
      types [N] int32, node_ptr [B + 1] int64, n_types T, qvec [Q, 3] int32 (the integer triples n; q = 2 pi n C^-T), rho [B, T, Q, 2]
      float64 (the modes of the last frame, (re, im)), frames [B] int64, cell_sum [B, 9] float64, flag [B] int32 (bits SQ_NOT_PERIODIC,
      SQ_NO_VOLUME, SQ_BAD_TYPE), sq_sum [B, P, Q] float64 with P = T (T + 1) / 2 — the unordered pair (a <= b) at pair_index(a, b);
      with fqt: n_lags, origins [K, B, T, Q, 2] float64 (the ring; the caller stores an origin with origins[k].copy_(rho)), fqt_sum
      [B, P, n_lags, Q] float64, fqt_count [B, n_lags] int64 — without: n_lags 0, origins [0, B, T, Q, 2], fqt_sum and fqt_count None."""

    __slots__ = ("types", "node_ptr", "n_types", "qvec", "rho", "frames", "cell_sum", "flag", "sq_sum", "n_lags", "origins", "fqt_sum",
                 "fqt_count")

    def pair_index(self, a, b):
        return _pair_index(a, b, self.n_types)


def sq_state(types, node_ptr, n_types=None, sq=None, device=None):
    """A fresh SqState.  types [N] integers in 0 .. n_types - 1 (n_types None: the largest type + 1) and node_ptr [B + 1], arrays or
    tensors, looked at here once as in observe_state; sq: dict(q | n_max[, fqt, max_bytes]) (ops.sq_numbers; the schedule of the
    ring is the caller's: ops.msd_schedule).  Every argument error — the byte budget among them — raises before a device or the
    library is asked for anything and before anything is allocated."""
    who = "sq_state"
    if sq is None:
        raise MdlError("%s: sq must be dict(q | n_max[, fqt, max_bytes])" % who)
    sq_numbers(who, n_types, sq)
    th, ph, N, B, T = _state_atoms(who, types, node_ptr, n_types)
    sq = sq_numbers(who, T, sq, B)
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    st = SqState()
    st.types = (types.detach().to(dev, torch.int32) if torch.is_tensor(types) else th.to(torch.int32).to(dev)).contiguous()
    st.node_ptr = (node_ptr.detach().to(dev, torch.int64) if torch.is_tensor(node_ptr) else ph.to(dev)).contiguous()
    st.n_types, st.qvec = T, torch.from_numpy(sq["q"]).to(dev)
    Q, P = st.qvec.shape[0], T * (T + 1) // 2
    z = lambda shape, dtype=torch.float64: torch.zeros(shape, dtype=dtype, device=dev)
    st.rho, st.frames, st.cell_sum, st.flag = z((B, T, Q, 2)), z((B,), torch.int64), z((B, 9)), z((B,), torch.int32)
    st.sq_sum = z((B, P, Q))
    fqt = sq["fqt"]
    st.n_lags = 0 if fqt is None else fqt["n_lags"]
    st.origins = z((0 if fqt is None else fqt["n_origins"], B, T, Q, 2))
    st.fqt_sum, st.fqt_count = (None, None) if fqt is None else (z((B, P, st.n_lags, Q)), z((B, st.n_lags), torch.int64))
    return st


def _sq_common(who, state, status):
    if not isinstance(state, SqState):
        raise MdlError("%s: state must be an ops.SqState (ops.sq_state)" % who)
    N, B = state.types.numel(), state.node_ptr.numel() - 1
    T, Q = int(state.n_types), (state.qvec.shape[0] if torch.is_tensor(state.qvec) and state.qvec.dim() == 2 else -1)
    if T > SQ_MAX_TYPES:
        raise MdlError("%s: at most %d types (got %d)" % (who, SQ_MAX_TYPES, T))
    if state.qvec.dtype != torch.int32 or tuple(state.qvec.shape) != (Q, 3) or not state.qvec.is_contiguous():
        raise MdlError("%s: state.qvec must be a contiguous [Q, 3] int32 tensor (got %s %s)" % (who, tuple(state.qvec.shape), state.qvec.dtype))
    if state.rho.dtype != torch.float64 or tuple(state.rho.shape) != (B, T, Q, 2) or not state.rho.is_contiguous():
        raise MdlError("%s: state.rho must be a contiguous [B, T, Q, 2] = %s float64 tensor (got %s %s)"
                       % (who, (B, T, Q, 2), tuple(state.rho.shape), state.rho.dtype))
    if status is not None and (not torch.is_tensor(status) or status.dtype != torch.int32 or tuple(status.shape) != (B,)
                               or not status.is_contiguous()):
        raise MdlError("%s: status must be a contiguous [B] int32 tensor with B = %d, or None" % (who, B))
    return N, B, T, Q


def density_modes(pos, cell, pbc, state, status=None):
    """The density modes of one frame of a batch: ONE launch, no host read (include/mdl_hip_scattering.h, mdl_density_modes).
      pos [N, 3] float64, unwrapped; cell [B, 3, 3] float64, rows are lattice vectors; pbc [B] int32, one bit per periodic axis; state
      an SqState (its types, node_ptr and qvec are used); status [B] int32 or None: structures with a non-zero status are skipped.
    state.rho[b, t, q] = the sum over the atoms of type t of exp(-2 pi i n_q . f), f = x C^-1 the fractional coordinates — a plain
    sum in ascending atom index, one sincospi per term; state.frames[b] += 1 and state.cell_sum[b] += cell[b].  A structure that is
    not periodic along all three axes or whose cell has no volume gets a bit in state.flag, is not counted and stays out of every
    later call; its rho, like that of a stopped or empty structure, keeps its bits.  No atomics: the same bits on every run, alone
    and in any batch.  Returns state."""
    who = "density_modes"
    N, B, T, Q = _sq_common(who, state, status)
    if not torch.is_tensor(pos) or pos.dtype != torch.float64 or pos.dim() != 2 or pos.shape[1] != 3 or not pos.is_contiguous():
        raise MdlError("%s: pos must be a contiguous [N, 3] float64 tensor (got %s %s)"
                       % (who, tuple(getattr(pos, "shape", ())), getattr(pos, "dtype", type(pos))))
    if pos.shape[0] != N:
        raise MdlError("%s: pos must be [N, 3] with N = %d, the atoms of the state (got %s)" % (who, N, tuple(pos.shape)))
    if not torch.is_tensor(cell) or cell.dtype != torch.float64 or tuple(cell.shape) != (B, 3, 3) or not cell.is_contiguous():
        raise MdlError("%s: cell must be a contiguous [B, 3, 3] float64 tensor with B = %d" % (who, B))
    if not torch.is_tensor(pbc) or pbc.dtype != torch.int32 or tuple(pbc.shape) != (B,) or not pbc.is_contiguous():
        raise MdlError("%s: pbc must be a contiguous [B] int32 tensor (one bit per axis) with B = %d" % (who, B))
    require_hip(pos, cell, pbc, status, state.qvec, state.rho)
    if any(t.device != pos.device for t in (cell, pbc, state.qvec, state.rho) + (() if status is None else (status,))):
        raise MdlError("%s: pos, cell, pbc, status and the state must be on one device" % who)
    check(lib().mdl_density_modes(ptr(pos), ptr(state.types), ptr(state.node_ptr), ptr(cell), ptr(pbc), ptr(status), ptr(state.qvec), N, B, Q,
                                  T, ptr(state.rho), ptr(state.frames), ptr(state.cell_sum), ptr(state.flag), stream()), "mdl_density_modes")
    return state


def sq_accumulate(lag, state, status=None):
    """state.rho — the modes density_modes has just written — into the structure factors of a batch: ONE launch, no host read
    (include/mdl_hip_scattering.h, mdl_sq_accumulate).
      lag [K] int32 ON THE DEVICE, one per slot of the ring state.origins: how many samples ago origins[k] was stored, negative: skip
      the slot (a row of ops.msd_schedule's table; live slots must have distinct lags), or None for a state without fqt (K = 0);
      status [B] int32 or None.
    Per pair of types (a <= c) and q, with R = rho and O an origin: w = 0.5 ((R_a.re O_c.re + R_a.im O_c.im) + (R_c.re O_a.re + R_c.im
    O_a.im)); state.sq_sum[b, pair, q] += w of O = R, at every call; state.fqt_sum[b, pair, lag[k], q] += w of O = origins[k, b] and
    state.fqt_count[b, lag[k]] += 1 for every live slot.  Stopped, empty and fatally flagged structures are skipped.  No atomics, a
    fixed expression per word: reproducible to the bit.  Returns state."""
    who = "sq_accumulate"
    N, B, T, Q = _sq_common(who, state, status)
    K = state.origins.shape[0]
    if K == 0:
        if lag is not None and not (torch.is_tensor(lag) and lag.numel() == 0):
            raise MdlError("%s: the state has no ring of origins (made without fqt): lag must be None" % who)
        lag = None
    elif not torch.is_tensor(lag) or lag.dtype != torch.int32 or tuple(lag.shape) != (K,) or not lag.is_contiguous():
        raise MdlError("%s: lag must be a contiguous [K] int32 tensor with K = %d, the slots of state.origins" % (who, K))
    require_hip(state.rho, lag, status, state.sq_sum)
    if any(t.device != state.rho.device for t in (lag, status) if t is not None):
        raise MdlError("%s: lag, status and the state must be on one device" % who)
    check(lib().mdl_sq_accumulate(ptr(state.rho), ptr(state.origins) if K else None, ptr(lag), ptr(state.flag), ptr(status), ptr(state.node_ptr),
                                  N, B, K, T, Q, max(int(state.n_lags), 1), ptr(state.sq_sum), ptr(state.fqt_sum), ptr(state.fqt_count),
                                  stream()), "mdl_sq_accumulate")
    return state
