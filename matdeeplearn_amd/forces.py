"""Forces from atomic positions: F = -dE/dpos through  positions -> minimum-image distances -> graph -> Gaussian expansion ->
CGCNN, SchNet, MEGNet or MPNN -> prediction, all of it on the HIP device.  The reference has no force path; this is the derivative
chain of the models the reference defines (matdeeplearn/models/) on the graphs it builds (matdeeplearn/process/process.py:258-305).

Chain, one public call (energy_and_forces):
  ops.build_graphs      neighbour lists — then HELD FIXED: forces are the derivative at fixed topology, as in every k-NN graph
                        potential (an atom that would enter or leave a neighbour list under the displacement does not)
  ops.edge_vectors      dist(pos) of those edges, bitwise the builder's distances; backward = csrc/edge_geom.hip
  (d - min) / (max - min)  the training set's normalisation (GraphDataset.dist_range)
  ops.rbf_expand + models.CGCNN with ops.cgconv(dist=...): every layer's backward returns dL/dd from the fused distance epilogue
                        of csrc/cgconv_de.hip — no [E, G] gradient is stored (fused=False: the general path through an [E, G]
                        edge-feature gradient per layer and mdl_rbf_expand_bwd, for comparison)
  models.SchNet with ops.cfconv(dist=...): the same through csrc/cfconv_de.hip, plus the second route — the cosine cutoff of the
                        RAW distance scales every message, so edge_weight carries a gradient and every block returns dL/dcut
  models.MEGNet / models.MPNN: the distance enters through one kind of layer only, a Linear(G -> M) + ReLU on the expansion —
                        the first layer of MEGNet's e_embed_list[0] (once), the first layer of every NNConv's edge network
                        (once per layer).  ops.rbf_linear_act puts a node behind that layer whose backward returns dL/dd from
                        csrc/linear_de.hip; everything behind it (gathers, scatters, BatchNorm, nnconv_msg, the GRU gates) is
                        differentiable in its inputs as it is
The derivative w.r.t. the cell (energy_forces_stress): at fixed neighbour lists and images a homogeneous strain eps maps every
edge displacement v to (I + eps) v, and d|v|/d eps_ab = v_a v_b / |v|, so dE/d eps_ab of structure b = sum over its edges of
(dE/dd_e) d_e u_e,a u_e,b — one reduction (ops.edge_strain_grad, csrc/edge_geom.hip) over the gradient w.r.t. the distances that
the same backward already forms, not a second derivative chain.
No second derivatives (training on forces): every backward is once_differentiable."""
import numpy as np
import torch

from . import ops
from .process import graph as pg
from .process.dataset import Batch


def _packed(structs):
    if isinstance(structs, dict):
        need = ("pos", "numbers", "node_ptr", "cell", "pbc")
        if any(k not in structs for k in need):
            raise ops.MdlError("energy_and_forces: packed arrays need the keys %s (process.graph.pack_structures)" % (need,))
        return structs
    return pg.pack_structures(structs)


def _host(a, dtype):
    return np.asarray(a.detach().cpu() if torch.is_tensor(a) else a, dtype=dtype)


def _node_features(numbers, out_deg, max_neighbors, dictionary, dev):
    """x = [atom features | one-hot out-degree incl. the self loop], as process.dataset._from_structures_device builds it"""
    z = np.asarray(numbers, dtype=np.int64)
    uz = np.unique(z)
    if dictionary is not None:                                 # one table row per distinct Z (graph.atom_features)
        table = np.asarray([dictionary[str(int(v))] for v in uz], dtype=np.float32)
    else:
        table = pg.atom_features(uz)
    feats = torch.from_numpy(table).to(dev).index_select(0, torch.from_numpy(np.searchsorted(uz, z)).to(dev))
    deg = torch.zeros((len(z), max_neighbors + 2), dtype=torch.float32, device=dev)
    deg.scatter_(1, out_deg.long().unsqueeze(1), 1.0)
    return torch.cat([feats, deg], 1)


def energy_and_forces(model, structs, dist_range, radius=8.0, max_neighbors=12, dictionary=None, output_index=None, fused=True,
                      routes=("expansion", "cutoff")):
    """Prediction and forces F = -d(prediction)/d(positions) of a CGCNN, SchNet, MEGNet or MPNN.

    model        a matdeeplearn_amd.models.CGCNN, .SchNet, .MEGNet or .MPNN on a HIP device (GCN raises MdlError).  Its CURRENT
                 mode is used.  eval() is the meaningful one: in training mode BatchNorm's batch statistics couple the graphs of
                 a batch (an atom would feel forces from other structures) and dropout makes the energy a random function.
    structs      a list of dict(positions, numbers, cell, pbc), or the packed arrays of process.graph.pack_structures
    dist_range   (min, max) of the TRAINING set's distance normalisation (GraphDataset.dist_range)
    radius, max_neighbors, dictionary   as process.from_structures
    output_index for a model with several outputs: the one to differentiate (default: the sum over the outputs)
    fused        True: dL/dd from the fused distance epilogue of the edge-gradient kernel (MEGNet / MPNN: of the first edge
                 layer, csrc/linear_de.hip); False: through an [E, G] edge-feature gradient per layer (same result to rounding;
                 for comparison)

    routes       diagnostic (SchNet): which of the two ways the distance enters carries the derivative — "expansion" (the Gaussian
                 expansion that feeds the filter network) and / or "cutoff" (the cosine cutoff of the raw distance).  The default,
                 both, is the force; one alone is that route's share (the two shares add up to the force).  The other models
                 have the expansion route only: without "expansion" their forces are zero.

    Returns (pred [B] or [B, out] fp32, forces [N, 3] fp32, node_ptr [B + 1] int64), device tensors; atom n of structure b is row
    node_ptr[b] + n.  The neighbour lists are built once from the given positions and HELD FIXED under the derivative; the image
    shifts and the cell are constants too (the strain derivative: energy_forces_stress).  Forces of a graph sum to zero up to
    fp32 rounding; with ops.deterministic() two calls return the same bits."""
    pred, gpos, _, node_ptr, _ = _energy_gradients(model, structs, dist_range, radius, max_neighbors, dictionary, output_index, fused, routes,
                                                   False)
    return pred, (-gpos).float(), node_ptr


def energy_forces_stress(model, structs, dist_range, radius=8.0, max_neighbors=12, dictionary=None, output_index=None, fused=True,
                         routes=("expansion", "cutoff"), volume_normalised=True):
    """Prediction, forces and stress of a CGCNN, SchNet, MEGNet or MPNN: energy_and_forces (same arguments, same pred and forces)
    plus the derivative w.r.t. a homogeneous strain of each structure.

    Returns (pred, forces [N, 3] fp32, stress [B, 3, 3] fp32, node_ptr).  stress[b] = (1 / V_b) dE/d eps, tensile positive, with
    dE/d eps_ab = sum over the edges of b of (dE/dd_e) d_e u_e,a u_e,b at fixed neighbour lists and images (positions, cell and
    shifts deform together) and V_b = |a . (b x c)| of the fp64 cell.  A structure that is not periodic in all three directions,
    or whose cell has no volume, has no stress: its row is NaN.  volume_normalised=False returns dE/d eps itself (an energy) for
    every structure.  Symmetric to the bit; the gradient w.r.t. the distances is taken in the backward that gives the forces and
    covers both of SchNet's routes."""
    pred, gpos, strain, node_ptr, (cell, pbc) = _energy_gradients(model, structs, dist_range, radius, max_neighbors, dictionary, output_index,
                                                                  fused, routes, True)
    if volume_normalised:
        a, b, c = cell[:, 0], cell[:, 1], cell[:, 2]
        vol = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2])
               + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])).abs()
        periodic = (pbc != 0).all(1) if pbc.dim() == 2 else (pbc & 7) == 7
        has_volume = periodic & (vol > 0)
        inv = torch.where(has_volume, 1.0 / torch.where(has_volume, vol, torch.ones_like(vol)), torch.full_like(vol, float("nan")))
        strain = (strain.double() * inv.view(-1, 1, 1)).float()
    return pred, (-gpos).float(), strain, node_ptr


def _energy_gradients(model, structs, dist_range, radius, max_neighbors, dictionary, output_index, fused, routes, want_strain):
    """The body of energy_and_forces / energy_forces_stress: (pred, dE/dpos, dE/d eps [B, 3, 3] or None, node_ptr, (cell, pbc))"""
    from .models import CGCNN, MEGNet, MPNN, SchNet
    if not isinstance(model, (CGCNN, SchNet, MEGNet, MPNN)):
        raise ops.MdlError("energy_and_forces: forces are implemented for CGCNN and SchNet, MEGNet and MPNN (got %s); GCN's edge "
                           "weight is the raw distance inside a degree normalisation, which has no distance gradient here "
                           "(DESIGN.md)" % type(model).__name__)
    schnet = isinstance(model, SchNet)
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise ops.MdlError("energy_and_forces: the model must be a CGCNN, SchNet, MEGNet or MPNN on a HIP device (got %s)" % dev)
    lo, hi = float(dist_range[0]), float(dist_range[1])
    if not hi > lo:
        raise ops.MdlError("energy_and_forces: dist_range must be (min, max) with max > min")
    p = _packed(structs)
    pos = torch.from_numpy(_host(p["pos"], np.float64)).to(dev)
    node_ptr = torch.from_numpy(_host(p["node_ptr"], np.int64)).to(dev)
    cell = torch.from_numpy(_host(p["cell"], np.float64)).to(dev)
    pbc = torch.from_numpy(_host(p["pbc"], np.int32)).to(dev)
    N, B = pos.shape[0], node_ptr.numel() - 1

    with torch.no_grad():
        edge_ptr, src, tgt, _, out_deg = ops.build_graphs(pos, node_ptr, cell, pbc, radius, max_neighbors)
        E = src.numel()
        ncnt = node_ptr[1:] - node_ptr[:-1]
        shift = torch.repeat_interleave(node_ptr[:-1], edge_ptr[1:] - edge_ptr[:-1], output_size=E).to(torch.int32)
        src, tgt = (src + shift).contiguous(), (tgt + shift).contiguous()          # batch-global ids, CSR by target
        csr = ops.EdgeCSR(ops.csr_rowptr(tgt, N), src, tgt, None, N, E)
        x = _node_features(_host(p["numbers"], np.int64), out_deg, int(max_neighbors), dictionary, dev)
        batch_idx = torch.repeat_interleave(torch.arange(B, device=dev), ncnt, output_size=N)

    with torch.enable_grad():
        pos_g = pos.detach().requires_grad_(True)
        if want_strain:
            dist, unit = ops.edge_vectors(pos_g, node_ptr, cell, pbc, src, tgt, csr=csr, return_unit=True)
        else:
            dist = ops.edge_vectors(pos_g, node_ptr, cell, pbc, src, tgt, csr=csr)
        d_norm = (dist - lo) / (hi - lo)                       # fp32, the arithmetic of GraphDataset.dist_norm
        if "expansion" not in routes:
            d_norm = d_norm.detach()
        if schnet:
            G = model.conv_list[0].mlp[0].in_features
        elif isinstance(model, MEGNet):
            G = model.e_embed_list[0][0].in_features
        elif isinstance(model, MPNN):
            G = model.conv_list[0].nn[0].in_features
        else:
            G = model.conv_list[0].dim
        cd = model.compute_dtype
        offsets = ops.rbf_offsets(0.0, 1.0, G, dev)
        # SchNet's energy depends on the distance through the expansion AND through the cosine cutoff of the raw distance
        data = Batch(x=x, edge_weight=dist if schnet and "cutoff" in routes else dist.detach(), batch=batch_idx, y=None, u=torch.zeros(B, 3, device=dev), num_graphs=B,
                     csr=csr, num_nodes=N, num_edges=E)
        if fused:
            data.edge_attr = ops.rbf_expand(d_norm.detach(), 0.0, 1.0, G, 0.2, out_dtype=cd, offsets=offsets)
            data.dist = (d_norm, offsets, ops.rbf_coeff(0.0, 1.0, 0.2))
        else:
            data.edge_attr = ops.rbf_expand(d_norm, 0.0, 1.0, G, 0.2, out_dtype=cd, offsets=offsets)
        pred = model(data)
        if pred.dim() == 2 and output_index is not None:
            energy = pred[:, int(output_index)].sum()
        else:
            energy = pred.sum()
        if want_strain:                                        # dE/dd: the sum of every route's gradient, as the geometry's backward gets it
            gpos, gdist = torch.autograd.grad(energy, [pos_g, dist], allow_unused=True)
        else:
            (gpos,), gdist = torch.autograd.grad(energy, pos_g, allow_unused=True), None
        if gpos is None:                                       # no route carries the derivative (routes without "expansion")
            gpos = torch.zeros_like(pos_g)
        strain = None
        if want_strain:
            if gdist is None:
                gdist = torch.zeros_like(dist)
            strain = ops.edge_strain_grad(gdist, dist.detach(), unit, node_ptr, csr=csr)
    return pred.detach(), gpos, strain, node_ptr, (cell, pbc)
