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
No second derivatives (training on forces): every backward is once_differentiable.
Consumers of the forces: ForceField keeps the packed structures, the atom features and the neighbour lists on the device across
calls (the host pass above happens once), and relax moves the atoms downhill with it — one batched FIRE update per step in one
launch (ops.fire_step, csrc/relax.hip), every structure with its own time step and its own convergence latch.  relax_cell moves
the cell with the atoms: the same update over the atoms' rows and the three rows of the deformation gradient, driven by the strain
gradient of energy_forces_stress (ops.fire_cell_step), still one launch per step.  md follows the forces at a temperature: BAOAB,
NVE or Langevin, one launch per step too (ops.md_step, csrc/md.hip), with counter-based noise, so a structure's trajectory is the
same alone and in any batch; md_npt is md at a pressure: an isotropic barostat (stochastic cell rescaling), driven by the strain
gradient, inside the same launch (ops.md_cell_step).  neb finds the barrier between two minima: the images of nudged elastic bands are the structures of ONE
ForceField, the band force (improved tangent, springs, climbing image) of every image is one launch (csrc/neb.hip) and FIRE then
moves every band as one object (ops.neb_step: the band mode of mdl_fire_step); interpolate_band makes a band from two end points.
sample is md or md_npt with the trajectory's observables recorded on the way, as an Observe asks: per sampled step one launch for
the pair histograms of the whole batch over every periodic image (ops.rdf_accumulate) and one for the mean-squared displacements
against a ring of time origins (ops.msd_accumulate), both csrc/observe.hip behind include/mdl_hip_analysis.h, and plain copies for
stored frames; no host read, the run's bits unchanged.  Observations holds the accumulators and turns them into g(r), MSD and a
diffusion coefficient.  A Correlate is an Observe that also asks for the velocity autocorrelation: the on-step velocity is formed
from what lies on the device in front of the integrator launch (ops.md_onstep_velocity) and correlated against a ring of origins
(ops.vacf_accumulate), both csrc/vacf.hip behind include/mdl_hip_dynamics.h; Observations turns the sums into the VACF, the
vibrational density of states and a Green-Kubo diffusion coefficient.  A Scatter is a Correlate that also asks for reciprocal space:
the density modes of every type at reciprocal-lattice vectors of the structure's own cell (ops.density_modes) and their products with
themselves and with a ring of stored modes (ops.sq_accumulate), both csrc/sq.hip behind include/mdl_hip_scattering.h; Observations
turns the sums into partial static structure factors S(q) and intermediate scattering functions F(q, t)."""
import collections
import inspect
import math

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


def _atom_block(numbers, dictionary, dev):
    """the atom-table rows of x, gathered once per atom (the only part of x that needs the host: np.unique over Z)"""
    z = np.asarray(numbers, dtype=np.int64)
    uz = np.unique(z)
    if dictionary is not None:                                 # one table row per distinct Z (graph.atom_features)
        table = np.asarray([dictionary[str(int(v))] for v in uz], dtype=np.float32)
    else:
        table = pg.atom_features(uz)
    return torch.from_numpy(table).to(dev).index_select(0, torch.from_numpy(np.searchsorted(uz, z)).to(dev))


def _with_degree_block(feats, out_deg, max_neighbors):
    """x = [atom features | one-hot out-degree incl. the self loop]: the degree block follows the neighbour lists, on the device"""
    deg = torch.zeros((feats.shape[0], max_neighbors + 2), dtype=torch.float32, device=feats.device)
    deg.scatter_(1, out_deg.long().unsqueeze(1), 1.0)
    return torch.cat([feats, deg], 1)


def _node_features(numbers, out_deg, max_neighbors, dictionary, dev):
    """x = [atom features | one-hot out-degree incl. the self loop], as process.dataset._from_structures_device builds it"""
    return _with_degree_block(_atom_block(numbers, dictionary, dev), out_deg, max_neighbors)


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
        strain = _per_volume(strain, cell, pbc)
    return pred, (-gpos).float(), strain, node_ptr


def _per_volume(strain, cell, pbc):
    """dE/d eps [B, 3, 3] -> stress: divided by the fp64 cell volume; NaN rows where a structure has no volume or is not periodic"""
    a, b, c = cell[:, 0], cell[:, 1], cell[:, 2]
    vol = (a[:, 0] * (b[:, 1] * c[:, 2] - b[:, 2] * c[:, 1]) + a[:, 1] * (b[:, 2] * c[:, 0] - b[:, 0] * c[:, 2])
           + a[:, 2] * (b[:, 0] * c[:, 1] - b[:, 1] * c[:, 0])).abs()
    has_volume = _periodic_with_volume(pbc, vol)
    inv = torch.where(has_volume, 1.0 / torch.where(has_volume, vol, torch.ones_like(vol)), torch.full_like(vol, float("nan")))
    return (strain.double() * inv.view(-1, 1, 1)).float()


def _periodic_with_volume(pbc, vol):
    """[B] bool: the structures that have a stress, and whose cell relax_cell may move — periodic along all three axes (pbc [B, 3],
    or [B] with one bit per axis) and with a cell volume vol [B] > 0"""
    return ((pbc != 0).all(1) if pbc.dim() == 2 else (pbc & 7) == 7) & (vol > 0)


def _accepted(model, dist_range):
    """The checks every entry point starts with: (device, lo, hi) of an accepted model on a HIP device and a usable dist_range"""
    from .models import CGCNN, MEGNet, MPNN, SchNet
    if not isinstance(model, (CGCNN, SchNet, MEGNet, MPNN)):
        raise ops.MdlError("energy_and_forces: forces are implemented for CGCNN and SchNet, MEGNet and MPNN (got %s); GCN's edge "
                           "weight is the raw distance inside a degree normalisation, which has no distance gradient here "
                           "(DESIGN.md)" % type(model).__name__)
    dev = next(model.parameters()).device
    if dev.type != "cuda":
        raise ops.MdlError("energy_and_forces: the model must be a CGCNN, SchNet, MEGNet or MPNN on a HIP device (got %s)" % dev)
    lo, hi = float(dist_range[0]), float(dist_range[1])
    if not hi > lo:
        raise ops.MdlError("energy_and_forces: dist_range must be (min, max) with max > min")
    return dev, lo, hi


def _upload(p, dev):
    """positions, node_ptr, cell and pbc of packed structures as device tensors"""
    return (torch.from_numpy(_host(p["pos"], np.float64)).to(dev), torch.from_numpy(_host(p["node_ptr"], np.int64)).to(dev),
            torch.from_numpy(_host(p["cell"], np.float64)).to(dev), torch.from_numpy(_host(p["pbc"], np.int32)).to(dev))


def _held_lists(graphs, node_ptr, N):
    """What a force evaluation holds fixed, from ops.build_graphs' result: batch-global (src, tgt), their EdgeCSR and out_deg"""
    edge_ptr, src, tgt, _, out_deg = graphs
    E = src.numel()
    shift = torch.repeat_interleave(node_ptr[:-1], edge_ptr[1:] - edge_ptr[:-1], output_size=E).to(torch.int32)
    src, tgt = (src + shift).contiguous(), (tgt + shift).contiguous()              # batch-global ids, CSR by target
    return src, tgt, ops.EdgeCSR(ops.csr_rowptr(tgt, N), src, tgt, None, N, E), out_deg


def _batch_index(node_ptr, N):
    B = node_ptr.numel() - 1
    return torch.repeat_interleave(torch.arange(B, device=node_ptr.device), node_ptr[1:] - node_ptr[:-1], output_size=N)


def _energy_gradients(model, structs, dist_range, radius, max_neighbors, dictionary, output_index, fused, routes, want_strain):
    """The body of energy_and_forces / energy_forces_stress: (pred, dE/dpos, dE/d eps [B, 3, 3] or None, node_ptr, (cell, pbc))"""
    dev, lo, hi = _accepted(model, dist_range)
    p = _packed(structs)
    pos, node_ptr, cell, pbc = _upload(p, dev)
    N = pos.shape[0]
    with torch.no_grad():
        src, tgt, csr, out_deg = _held_lists(ops.build_graphs(pos, node_ptr, cell, pbc, radius, max_neighbors), node_ptr, N)
        x = _node_features(_host(p["numbers"], np.int64), out_deg, int(max_neighbors), dictionary, dev)
        batch_idx = _batch_index(node_ptr, N)
    pred, gpos, strain = _device_gradients(model, pos, node_ptr, cell, pbc, src, tgt, csr, x, batch_idx, lo, hi, output_index, fused, routes,
                                           want_strain)
    return pred, gpos, strain, node_ptr, (cell, pbc)


def _device_gradients(model, pos, node_ptr, cell, pbc, src, tgt, csr, x, batch_idx, lo, hi, output_index, fused, routes, want_strain):
    """The device half both paths share: (pred, dE/dpos, dE/d eps [B, 3, 3] or None) at the positions `pos` on the GIVEN neighbour
    lists (src, tgt batch-global, csr their EdgeCSR) with the node features x.  Nothing here touches the host."""
    from .models import MEGNet, MPNN, SchNet
    schnet = isinstance(model, SchNet)
    dev, N, B, E = pos.device, pos.shape[0], node_ptr.numel() - 1, src.numel()
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
    return pred.detach(), gpos, strain


class ForceField:
    """The force chain of energy_and_forces, resident on the device: structures are packed and uploaded ONCE, the neighbour lists
    are an object that is HELD across calls and rebuilt on request, and an evaluation touches the host nowhere.

        ff = ForceField(model, structs, dist_range)      # arguments as energy_and_forces; builds the first lists
        ff.positions     [N, 3] float64, the live positions (a device tensor; written in place by set_positions and by relax)
        ff.node_ptr      [B + 1] int64;  ff.cell [B, 3, 3] float64, the live cells (written in place by set_cell and by
                         relax_cell);  ff.pbc [B] int32
        ff.edges         (src, tgt) int32, batch-global, of the lists currently held
        ff.set_positions(p)    new positions; the lists are NOT touched
        ff.set_cell(c, scale_atoms=False)   new cells [B, 3, 3] (scale_atoms: the atoms keep their fractional coordinates); the
                               lists are NOT touched
        ff.rebuild()           neighbour lists, their CSR and the out-degree block of x from the current positions, on the device
                               (one number, the edge count, is read back)
        ff.evaluate(stress=False)   (pred, forces [N, 3] fp32[, stress [B, 3, 3] fp32]) at the current positions ON THE HELD LISTS

    Right after construction or a rebuild(), evaluate() returns the bits of energy_and_forces / energy_forces_stress on structures
    at ff.positions (the same launches on the same operands).  Between rebuilds the energy is the smooth function whose derivative
    the forces are: an atom that would enter or leave a list under the displacement does not; the minimum image of every held edge
    is still chosen anew from the positions.  The model's CURRENT mode is used, as in energy_and_forces."""

    def __init__(self, model, structs, dist_range, radius=8.0, max_neighbors=12, dictionary=None, output_index=None, fused=True):
        self._dev, self._lo, self._hi = _accepted(model, dist_range)
        self.model, self.radius, self.max_neighbors = model, float(radius), int(max_neighbors)
        self.output_index, self.fused = output_index, bool(fused)
        p = _packed(structs)
        node_ptr = _host(p["node_ptr"], np.int64)
        n_atoms = _host(p["pos"], np.float64).shape[0]
        if n_atoms < 1:
            raise ops.MdlError("build_graphs: no atoms")
        if node_ptr.ndim != 1 or node_ptr.size < 2 or node_ptr[0] != 0 or node_ptr[-1] != n_atoms or (np.diff(node_ptr) < 0).any():
            raise ops.MdlError("build_graphs: node_ptr must start at 0, be non-decreasing and end at N = %d" % n_atoms)
        self.positions, self.node_ptr, self.cell, self.pbc = _upload(p, self._dev)
        self._atoms = _atom_block(_host(p["numbers"], np.int64), dictionary, self._dev)
        self._batch = _batch_index(self.node_ptr, n_atoms)
        self.rebuild()

    @property
    def edges(self):
        return self._src, self._tgt

    def set_positions(self, positions):
        """Overwrite the live positions ([N, 3], a device tensor or anything numpy reads).  The neighbour lists stay as they are."""
        p = positions if torch.is_tensor(positions) else torch.from_numpy(np.asarray(positions, dtype=np.float64))
        if tuple(p.shape) != tuple(self.positions.shape):
            raise ops.MdlError("ForceField.set_positions: positions must be [N, 3] with N = %d (got %s)" % (self.positions.shape[0], tuple(p.shape)))
        self.positions.copy_(p.detach())

    def set_cell(self, cell, scale_atoms=False):
        """Overwrite the live cells ([B, 3, 3], rows are lattice vectors; a device tensor or anything numpy reads).  With
        scale_atoms=True the atoms keep their fractional coordinates, pos <- pos C_old^-1 C_new per structure, on the device
        (atoms of a structure whose old cell has no volume stay where they are).  The neighbour lists stay as they are."""
        c = cell if torch.is_tensor(cell) else torch.from_numpy(np.asarray(cell, dtype=np.float64))
        if tuple(c.shape) != tuple(self.cell.shape):
            raise ops.MdlError("ForceField.set_cell: cell must be [B, 3, 3] with B = %d (got %s)" % (self.cell.shape[0], tuple(c.shape)))
        new = c.detach().to(self.cell.device, torch.float64)
        if scale_atoms:
            with torch.no_grad():
                o = self.cell
                adj = torch.stack([torch.linalg.cross(o[:, 1], o[:, 2]), torch.linalg.cross(o[:, 2], o[:, 0]),
                                   torch.linalg.cross(o[:, 0], o[:, 1])], 2)        # columns: b x c, c x a, a x b = det * C_old^-1
                det = (o[:, 0] * adj[:, :, 0]).sum(1)
                ok = det != 0
                inv = adj / torch.where(ok, det, torch.ones_like(det)).view(-1, 1, 1)
                eye = torch.eye(3, dtype=torch.float64, device=o.device).expand_as(o)
                m = torch.where(ok.view(-1, 1, 1), torch.bmm(inv, new), eye)
                self.positions.copy_(torch.bmm(self.positions.unsqueeze(1), m.index_select(0, self._batch)).squeeze(1))
        self.cell.copy_(new)

    def rebuild(self):
        """Neighbour lists from the current positions (ops.build_graphs' launches), made batch-global, with their CSR and the
        node features whose out-degree block follows them.  Reads the edge count back; nothing else crosses to the host."""
        with torch.no_grad():
            pos, node_ptr, cell, pbc, G = ops._graph_args(self.positions, self.node_ptr, self.cell, self.pbc)
            edge_ptr, src, tgt, dist, out_deg = ops._build_graphs_launch(pos, node_ptr, cell, pbc, G, self.radius, self.max_neighbors)
            E = int(edge_ptr[-1])
            self._src, self._tgt, self._csr, _ = _held_lists((edge_ptr, src[:E], tgt[:E], None, out_deg), node_ptr, pos.shape[0])
            self._x = _with_degree_block(self._atoms, out_deg, self.max_neighbors)

    def evaluate(self, stress=False, volume_normalised=True):
        """(pred [B] or [B, out] fp32, forces [N, 3] fp32) at the current positions on the held lists; with stress=True also
        stress [B, 3, 3] fp32 as energy_forces_stress defines it (volume_normalised=False: dE/d eps itself)."""
        pred, gpos, strain = _device_gradients(self.model, self.positions, self.node_ptr, self.cell, self.pbc, self._src, self._tgt, self._csr,
                                               self._x, self._batch, self._lo, self._hi, self.output_index, self.fused,
                                               ("expansion", "cutoff"), bool(stress))
        if not stress:
            return pred, (-gpos).float()
        return pred, (-gpos).float(), _per_volume(strain, self.cell, self.pbc) if volume_normalised else strain


RelaxResult = collections.namedtuple("RelaxResult", "positions energy forces converged steps fmax node_ptr")


def relax(model, structs, dist_range, fmax=0.05, steps=200, rebuild_every=1, fixed=None, dt=0.1, dt_max=1.0, maxstep=0.2, n_min=5,
          f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, check_every=10, radius=8.0, max_neighbors=12, dictionary=None,
          output_index=None):
    """Move the atoms of a batch of structures downhill in the model's prediction: FIRE (unit masses) on the forces of a
    ForceField, every structure with its own time step and its own convergence, the whole step on the device.

    model, structs, dist_range, radius, max_neighbors, dictionary, output_index   as energy_and_forces; the model must be in
                  eval() (training-mode BatchNorm couples the structures of a batch: a converged structure would keep moving
                  in energy with the others) — MdlError otherwise
    fmax          a structure is converged once its largest per-atom force is below this (a number, or one per structure); it is
                  then frozen: its positions keep their bits while the others go on
    steps         at most this many updates
    rebuild_every 0: the neighbour lists of the initial positions are held throughout (the energy is one smooth function);
                  n >= 1: the lists are rebuilt before every n-th evaluation, the final one included
    fixed         [N] mask (tensor or array, non-zero: the atom does not move), or None
    dt, dt_max, maxstep, n_min, f_inc, f_dec, alpha, f_alpha   FIRE's constants (ops.fire_step; alpha is also alpha_start);
                  maxstep bounds the norm of a structure's whole displacement per step
    check_every   the loop asks the device whether every structure is done every this many steps (the only host read besides
                  the edge count at a rebuild); 0: never, all `steps` updates are launched

    Positions are not wrapped into the cell (the minimum image does not need it).  After the last update the forces are evaluated
    once more, so energy, forces and fmax belong to the returned positions on the lists then in force.
    Returns RelaxResult(positions [N, 3] float64, energy [B] or [B, out] fp32, forces [N, 3] fp32, converged [B] bool, steps [B]
    int32 (updates made per structure), fmax [B] fp32 (largest per-atom force on a free atom), node_ptr), device tensors.  With
    ops.deterministic() two calls return the same bits: the integrator itself has no atomics."""
    const = dict(n_min=n_min, f_inc=f_inc, f_dec=f_dec, alpha_start=alpha, f_alpha=f_alpha, dt_max=dt_max, maxstep=maxstep)
    ff, state, probe, (fmax_t,), (energy, f) = _relax("relax", model, structs, dist_range, (("fmax", fmax),), steps, rebuild_every, check_every,
                                                      fixed, dt, const, (radius, max_neighbors, dictionary, output_index))
    converged = (state.done != 0) | (probe.fmax_seen.double() < fmax_t)
    return RelaxResult(ff.positions, energy, f, converged, state.steps, probe.fmax_seen, ff.node_ptr)


CellRelaxResult = collections.namedtuple("CellRelaxResult", "positions cell energy forces stress converged steps fmax smax status node_ptr")


def _per_structure(v, B, dev, who, what):
    """a number or one value per structure -> [B] float64 on the device"""
    if torch.is_tensor(v) or np.ndim(v) > 0:
        t = (v.detach() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v, dtype=np.float64))).to(dev, torch.float64)
        if tuple(t.shape) != (B,):
            raise ops.MdlError("%s: %s must be a number or one value per structure, [%d] (got %s)" % (who, what, B, tuple(t.shape)))
        return t.contiguous()
    return torch.full((B,), float(v), dtype=torch.float64, device=dev)


def _relax(who, model, structs, dist_range, bounds, steps, rebuild_every, check_every, fixed, dt, const, ff_args, cell=None, band=None):
    """relax, relax_cell and neb (`who`) behind their arguments: the checks, the ForceField, the rebuild / evaluate / step loop and
    the evaluation at the returned geometry.  bounds: ((name, value), ...) of the convergence criteria; const: the constants of the
    step; cell: None (ops.fire_step on the forces alone), or relax_cell's (cell_free, cell_factor) (ops.fire_cell_step on forces
    and strain gradient); band: None, or neb's (band_ptr as a host array, spring, climb, climb_after) (ops.neb_step: the state
    and the bounds are then per BAND, the structures are the images).  Returns (the ForceField, the state, a probe — a copy of the
    state with every latch set, stepped once at the returned geometry: with every latch set the integrator writes its criteria
    from its own pass 1 and nothing else —, the bounds as [B] float64 tensors, what that last evaluation returned)."""
    _accepted(model, dist_range)
    if model.training:
        raise ops.MdlError("%s: the model must be in eval() mode — training-mode BatchNorm couples the structures of a batch "
                           "(and dropout makes the energy a random function)" % who)
    steps, rebuild_every, check_every = int(steps), int(rebuild_every), int(check_every)
    if steps < 0 or rebuild_every < 0 or check_every < 0:
        raise ops.MdlError("%s: steps, rebuild_every and check_every must be >= 0" % who)
    if cell is not None and not 0.0 < float(const["max_deform"]) < 1.0:
        raise ops.MdlError("%s: max_deform must be in (0, 1) (got %r)" % (who, const["max_deform"]))
    ff = ForceField(model, structs, dist_range, *ff_args)
    dev, N, B = ff.positions.device, ff.positions.shape[0], ff.node_ptr.numel() - 1
    n_state = B if band is None else len(band[0]) - 1           # what has a state and a bound: the structures, or neb's bands
    bounds = [_per_structure(v, n_state, dev, who, name) for name, v in bounds]
    if fixed is not None:
        fixed = (fixed.detach() if torch.is_tensor(fixed) else torch.from_numpy(np.asarray(fixed))).to(dev)
        if tuple(fixed.shape) != (N,):
            raise ops.MdlError("%s: fixed must be an [N] mask with N = %d (got %s)" % (who, N, tuple(fixed.shape)))
        fixed = (fixed != 0).to(torch.uint8)
    if band is not None:
        band_ptr, spring, climb, climb_after = band
        state = ops.neb_state(ff.node_ptr, torch.from_numpy(np.asarray(band_ptr, dtype=np.int64)).to(dev), fixed, dt, const["alpha_start"])
        spring = _per_structure(spring, n_state, dev, who, "spring")
        climb = _per_structure(climb, n_state, dev, who, "climb") != 0
    elif cell is None:
        state = ops.fire_state(B, dt, const["alpha_start"], dev)
    else:
        cell_free, cell_factor = cell
        c = ff.cell
        free = _periodic_with_volume(ff.pbc, (c[:, 0] * torch.linalg.cross(c[:, 1], c[:, 2])).sum(1).abs())
        if cell_free is not None:
            mask = (cell_free.detach() if torch.is_tensor(cell_free) else torch.from_numpy(np.asarray(cell_free))).to(dev)
            if tuple(mask.shape) != (B,):
                raise ops.MdlError("%s: cell_free must be a [B] mask with B = %d (got %s)" % (who, B, tuple(mask.shape)))
            free = free & (mask != 0)
        if cell_factor is not None:
            cell_factor = _per_structure(cell_factor, B, dev, who, "cell_factor")
        state = ops.fire_cell_state(ff.positions, ff.cell, ff.node_ptr, free, cell_factor, dt, const["alpha_start"])
    vel = torch.zeros_like(ff.positions)
    n_eval = 0

    def advance(st):
        """the lists rebuilt when due, one evaluation, one update of `st`"""
        nonlocal n_eval
        if n_eval > 0 and rebuild_every > 0 and n_eval % rebuild_every == 0:
            ff.rebuild()
        n_eval += 1
        if band is not None:
            out = ff.evaluate()
            ops.neb_step(ff.positions, vel, out[1], _scalar_energy(out[0], ff.output_index), ff.cell, ff.pbc, st, *bounds, spring,
                         climb & (st.steps >= climb_after), **const)
        elif cell is None:
            out = ff.evaluate()
            ops.fire_step(ff.positions, vel, out[1], ff.node_ptr, st, *bounds, fixed, **const)
        else:
            out = ff.evaluate(stress=True, volume_normalised=False)
            ops.fire_cell_step(ff.positions, ff.cell, vel, out[1], out[2], ff.node_ptr, st, *bounds, fixed, **const)
        return out

    for it in range(steps):
        advance(state)
        if check_every > 0 and (it + 1) % check_every == 0 and bool(state.done.all()):
            break
    probe = state.clone()
    probe.done.fill_(1)
    return ff, state, probe, bounds, advance(probe)


def relax_cell(model, structs, dist_range, fmax=0.05, smax=1e-3, steps=200, rebuild_every=1, fixed=None, cell_free=None, cell_factor=None,
               max_deform=0.5, dt=0.1, dt_max=1.0, maxstep=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, check_every=10,
               radius=8.0, max_neighbors=12, dictionary=None, output_index=None):
    """relax with the cell among the degrees of freedom: FIRE over the atoms and the cell of every structure, driven by the forces
    and the strain gradient of a ForceField, the whole step on the device (ops.fire_cell_step: one launch).

    Coordinates (include/mdl_hip.h, mdl_fire_cell_step): with C0 the cell at the start, the cell is C = C0 F^T and atom i sits at
    F s_i; the integrator moves the rows s_i and the three rows of W = cell_factor F with the generalised forces F^T f_i and
    -(1 / cell_factor) (dE/d eps) F^-T, mixing, time step and maxstep taken over all N + 3 rows of a structure together.

    model, structs, dist_range, steps, rebuild_every, fixed, check_every, radius, max_neighbors, dictionary, output_index and
    FIRE's constants   as relax (fixed atoms keep their s_i: they ride with the cell)
    fmax, smax    a structure is converged once its largest per-atom force is below fmax AND, where its cell is free, the largest
                  component of its stress, max_ab |dE/d eps_ab| / volume, is below smax (numbers, or one per structure).  smax is
                  in the model's energy unit per cubic Angstrom: for a model trained on eV the default 1e-3 is 0.16 GPa
    cell_free     [B] mask or None (every cell).  The cell of a structure moves only if the structure is periodic along all three
                  axes, its cell has a volume and this mask allows it; every other structure is relaxed as relax does it (the
                  same bits), and its cell comes back as it went in
    cell_factor   [B] > 0 or None (max(1, atoms of the structure)): the weight of the cell's rows, see ops.fire_cell_state
    max_deform    in (0, 1): the trust region.  An update that would take |F - I| (Frobenius) beyond it is not made; the structure
                  stops at its last accepted geometry with status 2.  Every F a kernel sees therefore has a smallest singular
                  value >= 1 - max_deform: no collapsing cell reaches the graph builder.  Restart from the result to go further

    After the last update energy, forces and stress are evaluated once more, so they belong to the returned positions and cell on
    the lists then in force.  Returns CellRelaxResult(positions [N, 3] float64, cell [B, 3, 3] float64, energy, forces [N, 3] fp32,
    stress [B, 3, 3] fp32 (volume-normalised as energy_forces_stress returns it: NaN rows for structures without one), converged [B]
    bool, steps [B] int32, fmax [B] fp32, smax [B] fp32 (max |stress| at the returned geometry; NaN where stress is), status [B]
    int32 (0 still moving, 1 converged, 2 stopped by the trust region), node_ptr), device tensors.  With ops.deterministic() two
    calls return the same bits."""
    const = dict(n_min=n_min, f_inc=f_inc, f_dec=f_dec, alpha_start=alpha, f_alpha=f_alpha, dt_max=dt_max, maxstep=maxstep,
                 max_deform=max_deform)
    ff, state, probe, (fmax_t, smax_t), (energy, f, strain) = _relax(
        "relax_cell", model, structs, dist_range, (("fmax", fmax), ("smax", smax)), steps, rebuild_every, check_every, fixed, dt, const,
        (radius, max_neighbors, dictionary, output_index), (cell_free, cell_factor))
    fm, sm = probe.fmax_seen.double(), probe.smax_seen.double()
    met = ((fm < fmax_t) | ~(fm > 0)) & ((state.cell_free == 0) | (sm < smax_t) | ~(sm > 0))
    converged = (state.done == 1) | met
    stress = _per_volume(strain, ff.cell, ff.pbc)
    smax_seen = torch.where(torch.isnan(stress).flatten(1).any(1), torch.full_like(probe.smax_seen, float("nan")), probe.smax_seen)
    return CellRelaxResult(ff.positions, ff.cell, energy, f, stress, converged, state.steps, probe.fmax_seen, smax_seen, state.done, ff.node_ptr)


NEBResult = collections.namedtuple("NEBResult", "positions energy forces band_forces converged steps fmax climber barrier tangent_force "
                                                "path node_ptr band_ptr")


def _scalar_energy(pred, output_index):
    """the energy whose negative gradient the forces are, [B] fp32: the prediction, the chosen output or the sum over the outputs"""
    if pred.dim() == 1:
        return pred
    return pred[:, int(output_index)] if output_index is not None else pred.sum(1)


def _min_image(d, cell, pbc):
    """displacements d [n, 3] wrapped to their minimum image: fractional coordinates rounded on the periodic axes (host, fp64)"""
    cell, per = np.asarray(cell, dtype=np.float64), np.broadcast_to(np.asarray(pbc, dtype=bool).reshape(-1), 3)
    if not per.any() or np.linalg.det(cell) == 0.0:
        return d
    f = d @ np.linalg.inv(cell)
    f[:, per] -= np.rint(f[:, per])
    return f @ cell


def interpolate_band(initial, final, n_images):
    """The n_images structures of a band from `initial` to `final` (dict(positions, numbers, cell, pbc) each), end points included:
    positions linear in the minimum-image displacement final - initial, numbers, cell and pbc those of `initial` (the last image
    is `final` up to lattice vectors).  Host numpy.  MdlError where the two differ in atom count, numbers, cell or pbc."""
    n_images = int(n_images)
    if n_images < 2:
        raise ops.MdlError("interpolate_band: n_images must be >= 2 (got %d)" % n_images)
    p0, p1 = np.asarray(initial["positions"], dtype=np.float64), np.asarray(final["positions"], dtype=np.float64)
    if p0.shape != p1.shape or p0.ndim != 2 or p0.shape[1] != 3:
        raise ops.MdlError("interpolate_band: initial and final must have the same atoms, [n, 3] positions (got %s and %s)" % (p0.shape, p1.shape))
    if not np.array_equal(np.asarray(initial["numbers"]), np.asarray(final["numbers"])):
        raise ops.MdlError("interpolate_band: initial and final differ in their atomic numbers")
    no_cell, no_pbc = np.zeros((3, 3)), np.zeros(3, dtype=bool)
    cells = [np.asarray(no_cell if s.get("cell") is None else s["cell"], dtype=np.float64).reshape(3, 3) for s in (initial, final)]
    pbcs = [np.broadcast_to(np.asarray(no_pbc if s.get("pbc") is None else s["pbc"], dtype=bool).reshape(-1), 3) for s in (initial, final)]
    if not np.array_equal(cells[0], cells[1]) or not np.array_equal(pbcs[0], pbcs[1]):
        raise ops.MdlError("interpolate_band: initial and final differ in cell or pbc")
    d = _min_image(p1 - p0, cells[0], pbcs[0])
    return [dict(initial, positions=p0 + (k / (n_images - 1)) * d) for k in range(n_images)]


def neb(model, bands, dist_range, fmax=0.05, steps=200, spring=1.0, climb=True, climb_after=0, rebuild_every=1, fixed=None, dt=0.1,
        dt_max=1.0, maxstep=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, check_every=10, radius=8.0, max_neighbors=12,
        dictionary=None, output_index=None):
    """Minimum-energy paths and saddle points in the model's prediction: nudged elastic bands (improved tangent, Henkelman &
    Jonsson, J. Chem. Phys. 113, 9978; climbing image, 113, 9901) over the forces of ONE ForceField that holds every image of
    every band, moved by FIRE with a band as one object — one evaluation and one call (ops.neb_step: the band force of every image
    in one launch, the update of every band in a second) per step.

    model, dist_range, rebuild_every, check_every, radius, max_neighbors, dictionary, output_index and FIRE's constants   as relax;
                  the model must be in eval().  With several outputs the energy of the band force is the chosen output, or the sum
    bands         a list of bands, each a list of structures (interpolate_band makes one from two end points): the images, all
                  with the same atoms in the same order; the first and the last image of a band stay where they are.  A band of
                  fewer than three images has nothing to move and comes back converged
    fmax          a band is converged once the largest per-atom band force over all its images is below this (a number, or one
                  per band); it is then frozen as relax freezes a structure
    steps         at most this many updates (a band moves with one time step: steps counts per band)
    spring        the spring constant along the tangent, a number or one per band (energy per length squared)
    climb         a number / bool or one per band: the interior image of largest energy (lowest index on ties) feels the true force
                  with its tangent component inverted and no spring, so it converges to the saddle point
    climb_after   climbing starts once a band has made this many updates
    fixed         [N] mask over the atoms of all images in order, or None; the atoms of the end images are fixed anyway
    maxstep       bounds the norm of a whole band's displacement per step

    Displacements between neighbouring images are wrapped to their minimum image: an atom must move less than half a cell height
    between neighbours.  Every image has its own neighbour lists (rebuilt together when due), so the energy along a band is only
    piecewise smooth: two images whose lists differ sit on different smooth functions, the fixed-topology caveat of
    energy_and_forces; rebuild_every=0 holds the lists of the initial band.  After the last update everything is evaluated once
    more, so the results belong to the returned positions.
    Returns NEBResult(positions [N, 3] float64, energy [I] fp32, forces [N, 3] fp32 (true), band_forces [N, 3] fp32, converged [B]
    bool, steps [B] int32, fmax [B] fp32 (largest per-atom band force), climber [B] int32 (image index in the batch, -1: none),
    barrier [B] fp32 (largest interior energy minus the first image's; NaN without an interior image), tangent_force [I] float64
    (F.t^), path [I] float64 (cumulative distance along the band), node_ptr [I + 1], band_ptr [B + 1] int64), device tensors.
    With ops.deterministic() two calls return the same bits."""
    who = "neb"
    bands = [list(b) for b in bands]
    if not bands:
        raise ops.MdlError("%s: bands must be a non-empty list of lists of structures" % who)
    band_ptr = np.concatenate([[0], np.cumsum([len(b) for b in bands])]).astype(np.int64)
    for b, band in enumerate(bands):
        counts = [len(np.asarray(s["positions"])) for s in band]
        if len(set(counts)) > 1:
            raise ops.MdlError("%s: the images of band %d have unequal atom counts %s" % (who, b, counts))
    if int(climb_after) < 0:
        raise ops.MdlError("%s: climb_after must be >= 0" % who)
    const = dict(n_min=n_min, f_inc=f_inc, f_dec=f_dec, alpha_start=alpha, f_alpha=f_alpha, dt_max=dt_max, maxstep=maxstep)
    ff, state, probe, (fmax_t,), (pred, f) = _relax(who, model, [s for band in bands for s in band], dist_range, (("fmax", fmax),), steps,
                                                    rebuild_every, check_every, fixed, dt, const,
                                                    (radius, max_neighbors, dictionary, output_index), None,
                                                    (band_ptr, spring, climb, int(climb_after)))
    energy = _scalar_energy(pred, output_index)
    fm = probe.fmax_seen.double()
    converged = (state.done != 0) | (fm < fmax_t) | ~(fm > 0)
    nan = torch.full((1,), float("nan"), dtype=energy.dtype, device=energy.device)
    spans = list(zip(band_ptr[:-1].tolist(), band_ptr[1:].tolist()))
    barrier = torch.cat([(energy[i0 + 1:i1 - 1].max() - energy[i0]).view(1) if i1 - i0 >= 3 else nan for i0, i1 in spans])
    path = torch.cat([probe.seg_len[i0:i1].cumsum(0) for i0, i1 in spans])
    return NEBResult(ff.positions, energy, f, probe.band_force, converged, state.steps, probe.fmax_seen, probe.climber, barrier,
                     probe.tangent_force, path, ff.node_ptr, state.band_ptr)


# eV, Angstrom and atomic mass units: the time unit is A sqrt(amu / eV) = 10.18 fs.  dt = 2 * EV_A_AMU.fs is two femtoseconds,
# kT = EV_A_AMU.kB * 300 is 300 K, for a model trained on eV with masses in amu.
Units = collections.namedtuple("Units", "fs kB")
_E, _AMU, _K = 1.602176634e-19, 1.66053906660e-27, 1.380649e-23          # C, kg, J / K (SI 2019; CODATA 2018)
EV_A_AMU = Units(fs=1e-15 / (1e-10 * math.sqrt(_AMU / _E)), kB=_K / _E)

MDResult = collections.namedtuple("MDResult", "positions velocities energy forces ekin steps status epot_trace ekin_trace node_ptr")


def md(model, structs, dist_range, masses, dt, steps, kT=0.0, gamma=0.0, kT_init=None, velocities=None, seed=0, fixed=None,
       rebuild_every=1, max_disp=0.5, check_every=0, radius=8.0, max_neighbors=12, dictionary=None, output_index=None):
    """Molecular dynamics of a batch of structures in the model's prediction: BAOAB on the forces of a ForceField, one evaluation
    and ONE integrator launch (ops.md_step) per step, every structure with its own time step, thermostat and random stream.

    model, structs, dist_range, fixed, radius, max_neighbors, dictionary, output_index   as relax; the model must be in eval()
    masses        [N], one per atom in the order of the packed structures (tensor or array), > 0.  Units are the caller's: kT in
                  the model's energy unit, masses and dt consistent with it (EV_A_AMU for eV, Angstrom, amu)
    dt, kT, gamma a number or one per structure: time step > 0, thermostat temperature >= 0, friction >= 0 (1 / time).  gamma = 0
                  is NVE: no random number is drawn, and prediction + ekin is conserved on held lists up to the integrator's
                  O(dt^2) oscillation; gamma > 0 is Langevin dynamics at kT
    steps         this many steps: steps + 1 evaluations, the last call of the integrator only closes the last kick
    velocities    [N, 3] initial velocities, or None: Maxwell-Boltzmann at kT_init (None: kT) with the momentum of every structure
                  removed (ops.md_velocities)
    seed          an integer s (structure b is keyed s + b) or one int64 per structure.  A structure's trajectory does not depend
                  on what else is in the batch as far as the integrator goes: its noise is counted by (atom, step)
    rebuild_every 0: the neighbour lists of the initial positions are held throughout (the energy is one smooth function);
                  n >= 1: the lists are rebuilt before every n-th evaluation
    max_disp      the guard: a step that would move an atom further than this (or to a non-finite place) is not made; the
                  structure stops at its last positions with status 2 while the others go on
    check_every   the loop asks the device whether every structure has stopped every this many steps (the only host read besides
                  the edge count at a rebuild, and one look at masses, dt, kT and gamma at the first step); 0: never

    Returns MDResult(positions [N, 3] float64, velocities [N, 3] float64, energy [B] or [B, out] fp32 and forces [N, 3] fp32 at
    those positions, ekin [B] float64, steps [B] int32, status [B] int32 (1 finished, 2 stopped by the guard, 0 still running:
    only where check_every ended the loop), epot_trace [steps + 1, B(, out)] fp32 and ekin_trace [steps + 1, B] float64 — row n:
    prediction and kinetic energy at the positions after n steps (NaN rows: evaluations not made) —, node_ptr), device tensors.
    With ops.deterministic() two calls return the same bits."""
    ff, vel, state, (energy, f), (epot_trace, ekin_trace) = _md("md", model, structs, dist_range, masses, dt, steps, kT, gamma, kT_init, velocities,
                                                                seed, fixed, rebuild_every, max_disp, check_every,
                                                                (radius, max_neighbors, dictionary, output_index))
    return MDResult(ff.positions, vel, energy, f, state.ekin, state.steps, state.status, epot_trace, ekin_trace, ff.node_ptr)


def _md(who, model, structs, dist_range, masses, dt, steps, kT, gamma, kT_init, velocities, seed, fixed, rebuild_every, max_disp, check_every,
        ff_args, baro=None, observe=None):
    """md and md_npt (`who`) behind their arguments: the checks, the ForceField, the velocities and the rebuild / evaluate / step
    loop.  baro: None (ops.md_step on the forces alone), or md_npt's (pressure, rate, max_strain) as [B] host arrays and a number
    (ops.md_cell_step on forces and strain gradient; the kernel writes ff.cell).  Returns (the ForceField, the velocities, the
    state, what the last evaluation returned, the traces: prediction and state.ekin — with baro also state.volume and
    state.pressure — at every evaluation).  observe: None (md, md_npt: the launches are what they were), or sample's _Observer: it is
    told the run once and called at every evaluation, before that step's integrator launch; it reads positions, cell and status.
    An observer that asks for velocities (observe.velocities: a Correlate with vacf or stored frames) is called a second time between
    the evaluation and the integrator launch, with vel, the force just evaluated, the state and dt: from these it forms the on-step
    velocity itself (ops.md_onstep_velocity) and writes nothing the integrator or the force field reads."""
    _accepted(model, dist_range)
    if model.training:
        raise ops.MdlError("%s: the model must be in eval() mode — training-mode BatchNorm couples the structures of a batch "
                           "(and dropout makes the energy a random function)" % who)
    steps, rebuild_every, check_every = int(steps), int(rebuild_every), int(check_every)
    if steps < 0 or rebuild_every < 0 or check_every < 0:
        raise ops.MdlError("%s: steps, rebuild_every and check_every must be >= 0" % who)
    ff = ForceField(model, structs, dist_range, *ff_args)
    dev, N, B = ff.positions.device, ff.positions.shape[0], ff.node_ptr.numel() - 1

    def per_atom(v, what, tail, dtype):
        t = (v.detach() if torch.is_tensor(v) else torch.from_numpy(np.asarray(v))).to(dev)
        if tuple(t.shape) != (N,) + tail:
            raise ops.MdlError("%s: %s must be %s with N = %d (got %s)" % (who, what, list((N,) + tail), N, tuple(t.shape)))
        return (t != 0).to(torch.uint8) if dtype == torch.uint8 else t.to(dtype).contiguous().clone()

    mass = per_atom(masses, "masses", (), torch.float64)
    fixed = None if fixed is None else per_atom(fixed, "fixed", (), torch.uint8)
    dt_t, kT_t, gamma_t = [_per_structure(v, B, dev, who, name) for name, v in (("dt", dt), ("kT", kT), ("gamma", gamma))]
    if torch.is_tensor(seed) or np.ndim(seed) > 0:
        seed_t = (seed.detach() if torch.is_tensor(seed) else torch.from_numpy(np.asarray(seed, dtype=np.int64))).to(dev, torch.int64).contiguous()
        if tuple(seed_t.shape) != (B,):
            raise ops.MdlError("%s: seed must be an integer or one per structure, [%d] (got %s)" % (who, B, tuple(seed_t.shape)))
    else:
        seed_t = torch.arange(B, dtype=torch.int64, device=dev) + int(seed)
    if velocities is None:
        vel = ops.md_velocities(mass, ff.node_ptr, kT_t if kT_init is None else _per_structure(kT_init, B, dev, who, "kT_init"), seed_t, fixed)
    else:
        vel = per_atom(velocities, "velocities", (3,), torch.float64)
    if baro is None:
        state, traced = ops.md_state(B, dev), ("ekin",)
    else:
        state, traced = ops.md_cell_state(B, dev), ("ekin", "volume", "pressure")
        pressure_t, rate_t = [_per_structure(v, B, dev, who, name) for name, v in (("pressure", baro[0]), ("rate", baro[1]))]
    n_steps = torch.full((B,), steps, dtype=torch.int32, device=dev)
    traces = None
    if observe is not None:
        observe.start(ff, mass, fixed, dt_t, steps, baro is not None)
    for it in range(steps + 1):
        if it > 0 and rebuild_every > 0 and it % rebuild_every == 0:
            ff.rebuild()
        if observe is not None:
            observe.sample(it, ff, state.status)
        out = ff.evaluate() if baro is None else ff.evaluate(stress=True, volume_normalised=False)
        if observe is not None and observe.velocities:
            observe.sample_velocities(it, vel, out[1], state, dt_t)
        if baro is None:
            ops.md_step(ff.positions, vel, out[1], mass, ff.node_ptr, state, dt_t, n_steps, gamma_t, kT_t, seed_t, fixed, max_disp)
        else:
            ops.md_cell_step(ff.positions, vel, ff.cell, out[1], out[2], mass, ff.node_ptr, state, dt_t, n_steps, pressure_t, rate_t, gamma_t,
                             kT_t, seed_t, fixed, max_disp, baro[2])
        if traces is None:
            traces = [torch.full((steps + 1,) + tuple(out[0].shape), float("nan"), dtype=out[0].dtype, device=dev)]
            traces += [torch.full((steps + 1, B), float("nan"), dtype=torch.float64, device=dev) for _ in traced]
        traces[0][it].copy_(out[0])
        for t, k in zip(traces[1:], traced):
            t[it].copy_(getattr(state, k))
        if check_every > 0 and (it + 1) % check_every == 0 and bool((state.status != 0).all()):
            break
    return ff, vel, state, out[:2], traces


# eV / A^3 per GPa: pressure = 0.1 * GPA is a kilobar, compressibility = 1 / (100 * GPA) that of a bulk modulus of 100 GPa
GPA = 1e9 * 1e-30 / _E

NPTResult = collections.namedtuple("NPTResult", "positions velocities cell energy forces ekin volume pressure steps status epot_trace "
                                                "ekin_trace volume_trace pressure_trace node_ptr")


def md_npt(model, structs, dist_range, masses, dt, steps, pressure, tau_p, compressibility, kT=0.0, gamma=0.0, kT_init=None, velocities=None,
           seed=0, fixed=None, rebuild_every=1, max_disp=0.5, max_strain=0.03, check_every=0, radius=8.0, max_neighbors=12, dictionary=None,
           output_index=None):
    """md at constant pressure: the same loop with an isotropic barostat inside the integrator's launch (ops.md_cell_step) —
    stochastic cell rescaling (Bernetti & Bussi, J. Chem. Phys. 153, 114107 (2020)) in eps = ln V, driven by the strain gradient
    that the backward for the forces already forms.  With gamma > 0 and kT > 0 it samples the isothermal-isobaric ensemble (to
    first order in dt: the forces of a step are those of the unscaled positions); with kT = 0 it is the Berendsen barostat.

    model, structs, dist_range, masses, dt, steps, kT, gamma, kT_init, velocities, seed, fixed, rebuild_every, max_disp,
    check_every, radius, max_neighbors, dictionary, output_index   as md
    pressure      the target pressure, any sign, a number or one per structure, in the model's energy unit per cubic Angstrom
                  (pressure = 1.0 * GPA is one gigapascal for a model trained on eV)
    tau_p, compressibility   > 0, a number or one per structure each: the barostat's relaxation time and the (estimated) isothermal
                  compressibility, 1 / pressure; only their ratio enters.  tau_p = math.inf switches the barostat of that structure
                  off: it gets the bits of md, and its cell comes back as it went in.  A finite tau_p on a structure that is not
                  periodic along all three axes raises MdlError
    max_strain    the barostat's guard: a step that would change ln V by more than this (or whose cell has no volume) is not made;
                  the structure stops at its last geometry with status 3.  0.03 is a 1 % linear change per step; max_disp then
                  bounds the thermal motion alone

    Returns NPTResult(positions, velocities [N, 3] float64, cell [B, 3, 3] float64, energy and forces [N, 3] fp32 at that geometry,
    ekin, volume, pressure [B] float64 (the instantaneous pressure (2 ekin - tr dE/d eps) / (3 volume) there), steps, status [B]
    int32 (1 finished, 2 stopped by max_disp, 3 stopped by max_strain, 0 still running), epot_trace [steps + 1, B(, out)] fp32,
    ekin_trace, volume_trace, pressure_trace [steps + 1, B] float64, node_ptr), device tensors.  No host read beyond md's.  With
    ops.deterministic() two calls return the same bits."""
    return _md_npt(None, model, structs, dist_range, masses, dt, steps, pressure, tau_p, compressibility, kT, gamma, kT_init, velocities, seed,
                   fixed, rebuild_every, max_disp, max_strain, check_every, radius, max_neighbors, dictionary, output_index)


def _md_npt(observe, model, structs, dist_range, masses, dt, steps, pressure, tau_p, compressibility, kT, gamma, kT_init, velocities, seed, fixed,
            rebuild_every, max_disp, max_strain, check_every, radius, max_neighbors, dictionary, output_index):
    """md_npt behind its arguments (observe: as _md)"""
    who = "md_npt"
    p = _packed(structs)
    B = len(_host(p["node_ptr"], np.int64)) - 1

    def per_structure(v, what, positive):
        t = _host(v, np.float64)
        if t.ndim == 0:
            t = np.full(B, float(t))
        if t.shape != (B,):
            raise ops.MdlError("%s: %s must be a number or one value per structure, [%d] (got %s)" % (who, what, B, t.shape))
        if positive and not (t > 0).all():                     # (a NaN is not)
            raise ops.MdlError("%s: %s must be > 0" % (who, what))
        return t

    tau, kappa = per_structure(tau_p, "tau_p", True), per_structure(compressibility, "compressibility", True)
    press = per_structure(pressure, "pressure", False)
    if not np.isfinite(kappa).all() or not np.isfinite(press).all():
        raise ops.MdlError("%s: compressibility and pressure must be finite" % who)
    if not float(max_strain) > 0.0:
        raise ops.MdlError("%s: max_strain must be > 0 (got %r)" % (who, max_strain))
    rate = np.where(np.isinf(tau), 0.0, kappa / tau)
    open_ = (_host(p["pbc"], np.int32) & 7) != 7
    if (open_ & (rate > 0)).any():
        raise ops.MdlError("%s: structures %s are not periodic along all three axes: they have no pressure (tau_p = math.inf switches "
                           "their barostat off)" % (who, np.nonzero(open_ & (rate > 0))[0].tolist()))
    ff, vel, state, (energy, f), (epot_trace, ekin_trace, volume_trace, pressure_trace) = _md(
        who, model, p, dist_range, masses, dt, steps, kT, gamma, kT_init, velocities, seed, fixed, rebuild_every, max_disp, check_every,
        (radius, max_neighbors, dictionary, output_index), (press, rate, float(max_strain)), observe)
    return NPTResult(ff.positions, vel, ff.cell, energy, f, state.ekin, state.volume, state.pressure, state.steps, state.status, epot_trace,
                     ekin_trace, volume_trace, pressure_trace, ff.node_ptr)


# ------------------------------------------------------------------------------------------------
# Trajectory observables: what a run of md / md_npt leaves behind besides its last frame
# ------------------------------------------------------------------------------------------------
class Observe:
    """What forces.sample is to record along a run, all of it on the device (no host read, the run's bits unchanged):
      every         sample every this many steps (>= 1) ...
      skip          ... from this step on (>= 0): equilibration steps are not sampled.  Step `it` (0 .. steps, the positions after
                    `it` steps) is sampled if it >= skip and (it - skip) % every == 0
      rdf           None, or dict(r_max, nbins): the pair histogram of every structure out to r_max (every periodic image) in nbins
                    bins, per unordered pair of types
      msd           None, or dict(n_lags, origin_every, remove_com=True[, n_origins]): the mean-squared displacement per type at lags
                    of 0 .. n_lags - 1 SAMPLES against a ring of time origins, a new one every origin_every samples
                    (n_origins slots, by default ceil(n_lags / origin_every): every origin lives until its lag reaches n_lags);
                    remove_com: the displacement of the centre of mass of the structure's free atoms is taken out first
      frames_every  0, or store the positions (and, under NPT, the cells) of every this many steps — plain copies into [F, N, 3] /
                    [F, B, 3, 3] device tensors, F = steps // frames_every + 1
      types         None: one type per distinct atomic number of the batch, in sorted order; or an explicit [N] array of integers
                    >= 0 in the order of the packed structures
    The numbers are checked here; what needs the structures (the length of types, T (T + 1) / 2 * nbins against the kernel's
    histogram) is checked by forces.sample before it asks a device for anything."""

    def __init__(self, every=1, skip=0, rdf=None, msd=None, frames_every=0, types=None):
        self.every, self.skip, self.frames_every = int(every), int(skip), int(frames_every)
        if self.every < 1 or self.skip < 0 or self.frames_every < 0:
            raise ops.MdlError("Observe: every must be >= 1, skip and frames_every >= 0 (got %r, %r, %r)" % (every, skip, frames_every))
        self.rdf, self.msd = ops.observe_numbers("Observe", None, rdf, msd)
        self.types = None
        if types is not None:
            t = np.asarray(types.detach().cpu() if torch.is_tensor(types) else types)
            if t.ndim != 1 or t.dtype.kind not in "iu":
                raise ops.MdlError("Observe: types must be a one-dimensional integer array (got %s %s)" % (t.shape, t.dtype))
            if t.size and int(t.min()) < 0:
                raise ops.MdlError("Observe: types must be >= 0 (got %d)" % int(t.min()))
            self.types = t.astype(np.int64)


class Correlate(Observe):
    """An Observe that also asks what the trajectory says about time: every, skip, rdf, msd, frames_every, types as Observe, and
      vacf          None, or dict(n_lags, origin_every, remove_com=True[, n_origins]), ranges and defaults as msd: the velocity
                    autocorrelation per type at lags of 0 .. n_lags - 1 samples against a ring of time origins; remove_com: the
                    velocity of the centre of mass of the structure's free atoms is taken out of both factors first
    The velocity is the ON-STEP velocity, the one at the evaluated positions (ops.md_onstep_velocity restates the integrator's closing
    half kick on the force just evaluated); with frames_every > 0 it is stored next to the positions (Observations.frames_vel)."""

    def __init__(self, every=1, skip=0, rdf=None, msd=None, frames_every=0, types=None, vacf=None):
        Observe.__init__(self, every, skip, rdf, msd, frames_every, types)
        self.vacf = ops.vacf_numbers("Correlate", None, vacf)


class Scatter(Correlate):
    """A Correlate that also asks what the trajectory says in reciprocal space: every, skip, rdf, msd, frames_every, types, vacf as
    Correlate, and
      sq            None, or dict(q=<[Q, 3] integer array> | n_max=<int >= 1>, fqt=None | dict(n_lags, origin_every[, n_origins]),
                    max_bytes=2^30): the partial static structure factors S_ab(q) at every sample, and with fqt the partial
                    intermediate scattering functions F_ab(q, t) at lags of 0 .. n_lags - 1 samples against a ring of time origins
                    (ranges and defaults as msd).  The wave vectors are reciprocal-lattice vectors q = 2 pi n C^-T of every
                    structure's own cell, given as integer triples n shared by the batch: q, or with n_max every non-zero triple
                    with max |n_k| <= n_max of the half space — n is kept if its first non-zero component is positive, n and -n
                    carry the same information — in lexicographic order, Q = ((2 n_max + 1)^3 - 1) / 2 (ops.sq_half_space).
                    max_bytes bounds the two large buffers, 8 B P n_lags Q + 16 K B T Q bytes.  At most ops.SQ_MAX_TYPES types.
    Out of scope: the self part F_s(q, t), total X-ray or neutron weighting of the partials, and structures that are not periodic
    along all three axes (they would need Cartesian q; they are flagged, Observations.sq_flag, and not counted)."""

    def __init__(self, every=1, skip=0, rdf=None, msd=None, frames_every=0, types=None, vacf=None, sq=None):
        Correlate.__init__(self, every, skip, rdf, msd, frames_every, types, vacf)
        self.sq = ops.sq_numbers("Scatter", None, sq)


class Observations:
    """What forces.sample recorded: device tensors and small torch helpers.
      hist [B, P, nbins] int64 (ordered pairs (i, j, image) per unordered type pair, P = T (T + 1) / 2), frames [B] int64 (frames
      counted per structure), vol_sum [B] float64 (sum of |det cell| over them), flag [B] int32 (ops.RDF_* bits: why a structure
      was not counted) — None without rdf;  msd_sum [B, T, n_lags] float64, msd_count [B, n_lags] int64 — None without msd;
      types [N] int32, species (the atomic number of every type, or None with explicit types), type_counts [B, T] (FREE atoms per
      type: what msd averages over), type_totals [B, T] (all atoms: what g normalises with);
      frames_pos [F, N, 3], frames_cell [F, B, 3, 3] (NPT only) float64 and frames_step [F] int64 (the step of every stored frame,
      -1: the loop ended before it) — None without frames_every;  lag_time [B] float64: dt * every, the time between two samples.
      With a forces.Correlate: vacf_sum [B, 2, T, n_lags] float64 (plane 0: the sum of u . u0 over the free atoms of a type, plane 1:
      of m u . u0) and vacf_count [B, n_lags] int64 — None without vacf;  frames_vel [F, N, 3] float64, the ON-STEP velocities of the
      stored frames (the rows of a structure that the integrator has stopped are those last formed for it) — None without
      frames_every or with a plain Observe.
      With a forces.Scatter: qvec [Q, 3] int32 (the integer triples n), sq_sum [B, P, Q] float64 (the sum over the counted frames of
      Re rho_a conj(rho_b), symmetrised, per unordered pair of types), sq_frames [B] int64, sq_flag [B] int32 (ops.SQ_* bits),
      cell_sum [B, 9] float64 (the sum of the cells of the counted frames) — None without sq;  fqt_sum [B, P, n_lags, Q] float64 and
      fqt_count [B, n_lags] int64 — None without sq's fqt."""

    def __init__(self, state, species, type_counts, type_totals, frames_pos, frames_cell, frames_step, lag_time, pbc, vacf_state=None,
                 frames_vel=None, *, qvec=None, sq_sum=None, sq_frames=None, sq_flag=None, cell_sum=None, fqt_sum=None, fqt_count=None):
        self._state, self.species, self.type_counts, self.type_totals = state, species, type_counts, type_totals
        self.frames_pos, self.frames_cell, self.frames_step, self.lag_time, self._pbc = frames_pos, frames_cell, frames_step, lag_time, pbc
        for k in ("hist", "frames", "vol_sum", "flag", "msd_sum", "msd_count", "types", "r_max", "nbins", "n_lags"):
            setattr(self, k, getattr(state, k))
        self.vacf_sum, self.vacf_count = (None, None) if vacf_state is None else (vacf_state.vacf_sum, vacf_state.vacf_count)
        self.frames_vel = frames_vel
        self.qvec, self.sq_sum, self.sq_frames, self.sq_flag, self.cell_sum = qvec, sq_sum, sq_frames, sq_flag, cell_sum
        self.fqt_sum, self.fqt_count = fqt_sum, fqt_count

    def _asked(self, what, field):
        if field is None:
            raise ops.MdlError("Observations.%s: the run was not asked for it (forces.Observe)" % what)

    def r(self):
        """[nbins] float64: the bin centres"""
        self._asked("r", self.hist)
        return (torch.arange(self.nbins, dtype=torch.float64, device=self.hist.device) + 0.5) * (self.r_max / self.nbins)

    def counts(self, a, b):
        """[B, nbins] float64: ordered pairs of types (a, b) per frame and bin — for a != b both (a, b) and (b, a) — NaN for a
        structure without a counted frame.  This is what a cluster or a slab has in the place of g."""
        self._asked("counts", self.hist)
        fr = self.frames.double()
        return self.hist[:, self._state.pair_index(a, b)].double() / torch.where(fr > 0, fr, torch.full_like(fr, float("nan"))).unsqueeze(1)

    def g(self, a, b):
        """[B, nbins] float64: the radial distribution function of types (a, b) per structure, hist / (frames N_a N_b / <V> shell
        volume) (a != b: over 2, hist holds both orders) with <V> = vol_sum / frames, the MEAN volume of the sampled frames — a
        choice: under NPT normalising frame by frame differs at second order in the volume fluctuation.  MdlError if a structure
        of the batch is not periodic along all three axes: it has no density (counts gives its pairs per frame)."""
        self._asked("g", self.hist)
        if ((self._pbc & 7) != 7).any():
            raise ops.MdlError("Observations.g: structures %s are not periodic along all three axes: they have no density (counts(a, b) "
                               "gives their pairs per frame)" % np.nonzero((self._pbc & 7) != 7)[0].tolist())
        edges = torch.arange(self.nbins + 1, dtype=torch.float64, device=self.hist.device) * (self.r_max / self.nbins)
        shell = (4.0 / 3.0) * math.pi * (edges[1:] ** 3 - edges[:-1] ** 3)
        fr = self.frames.double()
        density = fr * self.type_totals[:, int(a)].double() * self.type_totals[:, int(b)].double() / (self.vol_sum / fr)
        return self.hist[:, self._state.pair_index(a, b)].double() / (density.unsqueeze(1) * shell * (1.0 if int(a) == int(b) else 2.0))

    def msd(self, t):
        """[B, n_lags] float64: the mean-squared displacement of the free atoms of type t at lags of 0 .. n_lags - 1 samples
        (lag_time each), NaN where no sample reached the lag (msd_count == 0) or the structure has no free atom of the type"""
        self._asked("msd", self.msd_sum)
        n = self.msd_count.double() * self.type_counts[:, int(t)].double().unsqueeze(1)
        return torch.where(n > 0, self.msd_sum[:, int(t)] / n, torch.full_like(n, float("nan")))

    def diffusion(self, t, lag_lo, lag_hi):
        """[B] float64: the least-squares slope of msd(t) over the lags lag_lo .. lag_hi - 1 against time (lag * lag_time), over 6"""
        lag_lo, lag_hi = int(lag_lo), int(lag_hi)
        self._asked("diffusion", self.msd_sum)
        if not 0 <= lag_lo < lag_hi - 1 or lag_hi > self.n_lags:
            raise ops.MdlError("Observations.diffusion: need 0 <= lag_lo < lag_hi - 1 and lag_hi <= n_lags = %d" % self.n_lags)
        y = self.msd(t)[:, lag_lo:lag_hi]
        x = torch.arange(lag_lo, lag_hi, dtype=torch.float64, device=y.device).unsqueeze(0) * self.lag_time.unsqueeze(1)
        xc, yc = x - x.mean(1, keepdim=True), y - y.mean(1, keepdim=True)
        return (xc * yc).sum(1) / (xc * xc).sum(1) / 6.0

    def vacf(self, t, mass_weighted=False):
        """[B, n_lags] float64: the velocity autocorrelation <u(0) . u(n)> of the free atoms of type t (mass_weighted: <m u(0) . u(n)>)
        at lags of 0 .. n_lags - 1 samples (lag_time each): the sum over vacf_count · the free atoms of the type.  NaN where no
        sample reached the lag or the structure has no free atom of the type"""
        self._asked("vacf", self.vacf_sum)
        n = self.vacf_count.double() * self.type_counts[:, int(t)].double().unsqueeze(1)
        return torch.where(n > 0, self.vacf_sum[:, 1 if mass_weighted else 0, int(t)] / n, torch.full_like(n, float("nan")))

    def vdos(self, t, window=True):
        """(freq [B, n_lags], dos [B, n_lags]) float64: the vibrational density of states of the free atoms of type t, the cosine
        transform of their mass-weighted velocity autocorrelation.  With M = n_lags - 1, dt = lag_time, N_t the free atoms of the
        type, c_n = vacf(t, mass_weighted=True)[n] / [0] and w_n = cos^2(pi n / (2 M)) (a Hann window that ends at the last lag;
        window=False: w_n = 1):
            dos_k  = 4 (3 N_t) dt  sum''_n  w_n c_n cos(pi n k / M)          freq_k = k / (2 M dt),   k = 0 .. M
        a DCT-I, sum'' giving half weight to n = 0 and n = M.  By its inverse at n = 0, sum''_k dos_k / (2 M dt) = 3 N_t exactly: the
        density integrates (trapezoid rule over freq) to the degrees of freedom of the type.  A structure with a lag that no sample
        reached, or without a free atom of the type, gets a NaN row.  Needs n_lags >= 2."""
        self._asked("vdos", self.vacf_sum)
        n_lags = self.vacf_sum.shape[-1]
        if n_lags < 2:
            raise ops.MdlError("Observations.vdos: needs n_lags >= 2 (got %d)" % n_lags)
        M = n_lags - 1
        c = self.vacf(t, mass_weighted=True)
        c = c / c[:, :1]
        n = torch.arange(n_lags, dtype=torch.float64, device=c.device)
        w = torch.cos(n * (math.pi / (2.0 * M))) ** 2 if window else torch.ones_like(n)
        w[0], w[M] = 0.5 * w[0], 0.5 * w[M]
        basis = torch.cos(torch.outer(n, n) * (math.pi / M))                        # [n, k]
        dt = self.lag_time.unsqueeze(1)
        dos = 4.0 * (3.0 * self.type_counts[:, int(t)].double().unsqueeze(1)) * dt * ((c * w) @ basis)
        return n.unsqueeze(0) / (2.0 * M * dt), dos

    def diffusion_gk(self, t, lag_hi):
        """[B] float64: the Green-Kubo diffusion coefficient of type t, a third of the trapezoid integral of vacf(t) over the lags
        0 .. lag_hi - 1 (lag * lag_time)"""
        lag_hi = int(lag_hi)
        self._asked("diffusion_gk", self.vacf_sum)
        if not 1 <= lag_hi <= self.vacf_sum.shape[-1]:
            raise ops.MdlError("Observations.diffusion_gk: need 1 <= lag_hi <= n_lags = %d" % self.vacf_sum.shape[-1])
        y = self.vacf(t)[:, :lag_hi]
        return (y.sum(1) - 0.5 * (y[:, 0] + y[:, -1])) * self.lag_time / 3.0

    def q(self):
        """[B, Q, 3] float64: the wave vectors q = 2 pi n (C^-1)^T of every structure, with C = cell_sum / sq_frames, the MEAN cell of
        the counted frames — exact at constant volume, a choice under NPT (as g takes the mean volume): the modes of every frame
        were taken at that frame's own reciprocal lattice, the same integers n.  NaN for a structure without a counted frame."""
        self._asked("q", self.sq_sum)
        fr = self.sq_frames.double()
        C = (self.cell_sum / torch.where(fr > 0, fr, torch.full_like(fr, float("nan"))).unsqueeze(1)).view(-1, 3, 3)
        # the rows of (C^-1)^T are the reciprocal vectors a_j x a_k / det
        rec = torch.stack([torch.linalg.cross(C[:, (k + 1) % 3], C[:, (k + 2) % 3]) for k in range(3)], 1)
        rec = rec / (C[:, 0] * rec[:, 0]).sum(1).view(-1, 1, 1)
        return (2.0 * math.pi) * torch.einsum("qk,bkc->bqc", self.qvec.double(), rec)

    def q_norm(self):
        """[B, Q] float64: |q| of every wave vector (Observations.q)"""
        return self.q().norm(dim=2)

    def _sq_norm(self, a, b):
        n = self.type_totals[:, int(a)].double() * self.type_totals[:, int(b)].double()
        return torch.where(n > 0, n.sqrt(), torch.full_like(n, float("nan")))

    def sq(self, a, b):
        """[B, Q] float64: the Ashcroft-Langreth partial structure factor S_ab(q) = < Re rho_a(q) conj(rho_b(q)) > / sqrt(N_a N_b) of
        types (a, b) at the vectors of qvec: sq_sum / (sq_frames sqrt(N_a N_b)) with N from type_totals (fixed atoms scatter like any
        other).  NaN for a structure without a counted frame or without atoms of one of the types."""
        self._asked("sq", self.sq_sum)
        pair = ops._pair_index(a, b, self.type_totals.shape[1])
        fr = self.sq_frames.double()
        n = torch.where(fr > 0, fr, torch.full_like(fr, float("nan"))) * self._sq_norm(a, b)
        return self.sq_sum[:, pair] / n.unsqueeze(1)

    def sq_radial(self, a, b, q_max, nbins):
        """(centres [nbins], S [B, nbins]) float64: sq(a, b) averaged over the vectors whose |q| (q_norm) falls into each of nbins
        shells of width q_max / nbins from 0, per structure; NaN for a shell without a vector"""
        q_max, nbins = float(q_max), int(nbins)
        self._asked("sq_radial", self.sq_sum)
        if not (q_max > 0.0 and q_max < float("inf")) or nbins < 1:
            raise ops.MdlError("Observations.sq_radial: need q_max > 0, finite, and nbins >= 1 (got %r, %r)" % (q_max, nbins))
        s, qn = self.sq(a, b), self.q_norm()
        inside = torch.isfinite(qn) & (qn < q_max)
        idx = torch.where(inside, (qn * (nbins / q_max)).floor(), torch.zeros_like(qn)).long().clamp_(0, nbins - 1)
        total = torch.zeros((s.shape[0], nbins), dtype=torch.float64, device=s.device).scatter_add_(1, idx, torch.where(inside, s, torch.zeros_like(s)))
        count = torch.zeros_like(total).scatter_add_(1, idx, inside.double())
        centres = (torch.arange(nbins, dtype=torch.float64, device=s.device) + 0.5) * (q_max / nbins)
        return centres, torch.where(count > 0, total / count, torch.full_like(total, float("nan")))

    def fqt(self, a, b):
        """[B, n_lags, Q] float64: the partial intermediate scattering function F_ab(q, t) = < Re rho_a(q, t0 + t) conj(rho_b(q, t0)) >
        / sqrt(N_a N_b), symmetrised in (a, b), at lags of 0 .. n_lags - 1 samples (lag_time each): fqt_sum / (fqt_count sqrt(N_a N_b)).
        NaN where no sample reached the lag (fqt_count == 0) or the structure has no atoms of one of the types."""
        self._asked("fqt", self.fqt_sum)
        pair = ops._pair_index(a, b, self.type_totals.shape[1])
        c = self.fqt_count.double()
        n = torch.where(c > 0, c, torch.full_like(c, float("nan"))) * self._sq_norm(a, b).unsqueeze(1)
        return self.fqt_sum[:, pair] / n.unsqueeze(2)


class _Observer:
    """forces.sample's side of _md's hook.  Everything that decides WHEN something is sampled is host arithmetic, done here once:
    the sampled steps, the ring of origins and the lag of every slot at every sample (ops.msd_schedule, uploaded as one table)."""

    def __init__(self, req, p, steps):
        who = "sample"
        z, node_ptr = _host(p["numbers"], np.int64), _host(p["node_ptr"], np.int64)
        N = len(z)
        if req.types is None:
            self.species = np.unique(z)
            self.types = np.searchsorted(self.species, z)
        else:
            if req.types.shape != (N,):
                raise ops.MdlError("%s: Observe.types must be [N] with N = %d (got %s)" % (who, N, req.types.shape))
            self.species, self.types = None, req.types
        self.T = int(self.types.max()) + 1 if N else 1
        self.rdf, self.msd = ops.observe_numbers(who, self.T, req.rdf, req.msd)
        self.vacf = ops.vacf_numbers(who, self.T, req.vacf) if isinstance(req, Correlate) else None
        # what _md's second hook is for: only a Correlate can ask, so a plain Observe keeps the launches it had
        self.velocities = isinstance(req, Correlate) and (self.vacf is not None or req.frames_every > 0)
        # only a Scatter can ask for structure factors: a plain Observe or Correlate keeps the launches it had
        self.sq = ops.sq_numbers(who, self.T, req.sq, len(node_ptr) - 1) if isinstance(req, Scatter) else None
        self.req, self.node_ptr, self.pbc = req, node_ptr, _host(p["pbc"], np.int32)
        self.sample_of = {it: s for s, it in enumerate(range(req.skip, int(steps) + 1, req.every))}
        self.state = None

    def start(self, ff, mass, fixed, dt, steps, npt):
        dev, N, B = ff.positions.device, ff.positions.shape[0], ff.node_ptr.numel() - 1
        self.state = ops.observe_state(self.types, self.node_ptr, self.T, self.rdf, self.msd, dev)
        self.mass, self.fixed = mass, fixed
        if self.msd is not None:
            slot, lag = ops.msd_schedule(len(self.sample_of), self.msd["n_lags"], self.msd["origin_every"], self.msd["n_origins"])
            self.slot, self.lag = slot.tolist(), lag.to(dev)
        flat = _batch_index(ff.node_ptr, N) * self.T + self.state.types.long()
        count = lambda w: torch.zeros(B * self.T, dtype=torch.int64, device=dev).index_add_(0, flat, w).view(B, self.T)
        ones = torch.ones(N, dtype=torch.int64, device=dev)
        self.type_totals, self.type_counts = count(ones), count(ones if fixed is None else (fixed == 0).long())
        self.lag_time = dt * float(self.req.every)
        self.frames_pos = self.frames_cell = self.frames_step = None
        if self.req.frames_every > 0:
            F = steps // self.req.frames_every + 1
            self.frames_pos = torch.full((F, N, 3), float("nan"), dtype=torch.float64, device=dev)
            self.frames_cell = torch.full((F, B, 3, 3), float("nan"), dtype=torch.float64, device=dev) if npt else None
            self.frames_step = [-1] * F
        self.vstate = self.frames_vel = None
        if self.velocities:
            self.ff_node_ptr = ff.node_ptr.contiguous()
            self.onstep = torch.zeros((N, 3), dtype=torch.float64, device=dev)
            if self.vacf is not None:
                self.vstate = ops.vacf_state(self.types, self.node_ptr, self.T, self.vacf, dev)
                slot, lag = ops.msd_schedule(len(self.sample_of), self.vacf["n_lags"], self.vacf["origin_every"], self.vacf["n_origins"])
                self.vslot, self.vlag = slot.tolist(), lag.to(dev)
            if self.req.frames_every > 0:
                self.frames_vel = torch.full((F, N, 3), float("nan"), dtype=torch.float64, device=dev)
        self.sstate = None
        if self.sq is not None:
            self.sstate = ops.sq_state(self.types, self.node_ptr, self.T, self.sq, dev)
            self.qslot = self.qlag = None
            if self.sq["fqt"] is not None:
                fqt = self.sq["fqt"]
                slot, lag = ops.msd_schedule(len(self.sample_of), fqt["n_lags"], fqt["origin_every"], fqt["n_origins"])
                self.qslot, self.qlag = slot.tolist(), lag.to(dev)

    def sample_velocities(self, it, vel, force, state, dt):
        """_md's second hook, between the evaluation of step `it` and its integrator launch: the on-step velocity, formed ONCE where
        a frame is stored or the step is sampled (one launch), a plain copy per frame and per new origin, one correlation launch"""
        every = self.req.frames_every
        frame = every > 0 and it % every == 0
        s = self.sample_of.get(it) if self.vstate is not None else None
        if not frame and s is None:
            return
        ops.md_onstep_velocity(vel, force.contiguous(), self.mass, self.ff_node_ptr, state, dt, self.fixed, self.onstep)
        if frame:
            self.frames_vel[it // every].copy_(self.onstep)
        if s is not None:
            if self.vslot[s] >= 0:
                self.vstate.origins[self.vslot[s]].copy_(self.onstep)
            ops.vacf_accumulate(self.onstep, self.vlag[s], self.mass, self.vstate, self.fixed, state.status, self.vacf["remove_com"])

    def sample(self, it, ff, status):
        every = self.req.frames_every
        if every > 0 and it % every == 0:
            self.frames_pos[it // every].copy_(ff.positions)
            if self.frames_cell is not None:
                self.frames_cell[it // every].copy_(ff.cell)
            self.frames_step[it // every] = it
        s = self.sample_of.get(it)
        if s is None:
            return
        if self.rdf is not None:
            ops.rdf_accumulate(ff.positions, ff.cell, ff.pbc, self.state, status)
        if self.msd is not None:
            if self.slot[s] >= 0:
                self.state.origins[self.slot[s]].copy_(ff.positions)
            ops.msd_accumulate(ff.positions, self.lag[s], self.mass, self.state, self.fixed, status, self.msd["remove_com"])
        if self.sstate is not None:
            # the modes of this frame (one launch), a plain copy where the schedule opens an origin, the products (one launch)
            ops.density_modes(ff.positions, ff.cell, ff.pbc, self.sstate, status)
            if self.qslot is not None and self.qslot[s] >= 0:
                self.sstate.origins[self.qslot[s]].copy_(self.sstate.rho)
            ops.sq_accumulate(None if self.qlag is None else self.qlag[s], self.sstate, status)

    def result(self):
        steps = None if self.frames_step is None else torch.tensor(self.frames_step, dtype=torch.int64, device=self.frames_pos.device)
        st = self.sstate
        sq = {} if st is None else dict(qvec=st.qvec, sq_sum=st.sq_sum, sq_frames=st.frames, sq_flag=st.flag, cell_sum=st.cell_sum,
                                        fqt_sum=st.fqt_sum, fqt_count=st.fqt_count)
        return Observations(self.state, self.species, self.type_counts, self.type_totals, self.frames_pos, self.frames_cell, steps,
                            self.lag_time, self.pbc, self.vstate, self.frames_vel, **sq)


def sample(model, structs, dist_range, masses, dt, steps, observe, npt=None, **md_kwargs):
    """forces.md or forces.md_npt with the trajectory's observables recorded on the way: the radial distribution function, the
    mean-squared displacement and stored frames, as `observe` (a forces.Observe) asks.  The run is the one md / md_npt make from the
    same arguments, to the bit: sampling reads positions, cells and status words between two steps and writes nothing the
    integrator or the force field reads.  Per SAMPLED step the loop makes one pair-histogram launch (ops.rdf_accumulate) and one
    displacement launch (ops.msd_accumulate) before that step's integrator launch, a plain copy where a time origin or a frame is
    stored, and nothing otherwise; no host read is added.

    model, structs, dist_range, masses, dt, steps   as md
    observe       forces.Observe(...)
    npt           None: md's loop;  dict(pressure, tau_p, compressibility[, max_strain]): md_npt's, with its checks
    md_kwargs     md's keyword arguments (kT, gamma, kT_init, velocities, seed, fixed, rebuild_every, max_disp, check_every, radius,
                  max_neighbors, dictionary, output_index)

    A structure that the integrator's guard has stopped (status != 0) stops contributing from the next sample on; the last
    evaluation (step == steps) is sampled if the schedule reaches it.  Positions are unwrapped throughout, which is what the
    displacement needs; the histogram reduces every pair to its nearest image itself.  Under NPT the barostat scales the
    positions with the cell, and the displacement is taken on the scaled coordinates AS THEY ARE: it contains the affine motion
    of the cell (small against diffusion at a stable volume; divide the frames by the cell to take it out).  g is normalised by
    the mean volume of the sampled frames (Observations.g).
    With a forces.Correlate (an Observe with vacf=...) the loop also records the velocity autocorrelation per type, and stores the
    velocities of the frames: on a sampled step, between the evaluation and the integrator launch, one launch forms the on-step
    velocity from vel, the force just evaluated, the masses, dt and the integrator's step words (ops.md_onstep_velocity: the closing
    half kick that the integrator itself applies only in its next call), a plain copy stores it where the schedule starts a new
    origin, and one launch correlates it with the ring (ops.vacf_accumulate); on a step that only stores a frame, the first launch
    and a copy.  Under NPT the velocity is the on-step velocity BEFORE the barostat's 1 / s scaling of that step.  Observations.vacf,
    .vdos and .diffusion_gk turn the sums into the correlation function, the vibrational density of states and a Green-Kubo
    diffusion coefficient.  With a plain Observe the launches are what they were.
    With a forces.Scatter (a Correlate with sq=...) the positions hook of a sampled step also makes one launch for the density modes
    of every type at the asked reciprocal-lattice vectors (ops.density_modes), a plain copy of them into the ring where the schedule
    opens an origin, and one launch for the products (ops.sq_accumulate): Observations.sq, .sq_radial, .fqt, .q and .q_norm turn the
    sums into partial structure factors and intermediate scattering functions.  With a plain Observe or Correlate the launches are
    what they were.
    Returns (MDResult or NPTResult, Observations).  Counts are integer sums and the displacement sums have no atomics: two calls
    return the same bits, and a structure's observables do not depend on the batch it is in as far as its trajectory does not."""
    who = "sample"
    if not isinstance(observe, Observe):
        raise ops.MdlError("%s: observe must be a forces.Observe (got %s)" % (who, type(observe).__name__))
    kw = {k: v.default for k, v in inspect.signature(md).parameters.items() if v.default is not inspect.Parameter.empty}
    unknown = sorted(set(md_kwargs) - set(kw))
    if unknown:
        raise ops.MdlError("%s: unknown keyword arguments %s (md's are %s)" % (who, unknown, sorted(kw)))
    kw.update(md_kwargs)
    if npt is not None:
        need, may = {"pressure", "tau_p", "compressibility"}, {"max_strain"}
        if not isinstance(npt, dict) or not need <= set(npt) <= need | may:
            raise ops.MdlError("%s: npt must be None or dict(pressure, tau_p, compressibility[, max_strain])" % who)
    p = _packed(structs)
    obs = _Observer(observe, p, steps)
    ff_args = (kw["radius"], kw["max_neighbors"], kw["dictionary"], kw["output_index"])
    if npt is None:
        ff, vel, state, (energy, f), (epot_trace, ekin_trace) = _md(
            "md", model, p, dist_range, masses, dt, steps, kw["kT"], kw["gamma"], kw["kT_init"], kw["velocities"], kw["seed"], kw["fixed"],
            kw["rebuild_every"], kw["max_disp"], kw["check_every"], ff_args, None, obs)
        res = MDResult(ff.positions, vel, energy, f, state.ekin, state.steps, state.status, epot_trace, ekin_trace, ff.node_ptr)
    else:
        res = _md_npt(obs, model, p, dist_range, masses, dt, steps, npt["pressure"], npt["tau_p"], npt["compressibility"], kw["kT"],
                      kw["gamma"], kw["kT_init"], kw["velocities"], kw["seed"], kw["fixed"], kw["rebuild_every"], kw["max_disp"],
                      npt.get("max_strain", 0.03), kw["check_every"], *ff_args)
    return res, obs.result()
