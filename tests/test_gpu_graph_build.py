"""GPU: the HIP graph builder (ops.build_graphs, process.from_structures(device=...)) against the host builder and the
reference's goldens — pt10 (non-periodic, reference-produced edges), orthorhombic clouds with ties and coincident atoms under
every pbc combination (bitwise), skewed triclinic cells (same edges, distances within 1 fp32 ulp), sizes from 1 to 2048 atoms,
dictionary features, determinism, argument errors, and one training epoch on the device-built dataset."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
G = os.path.join(os.path.dirname(__file__), "golden")
FIELDS = ("node_ptr", "edge_ptr", "x", "z", "src", "tgt", "dist", "dist_norm", "in_deg", "lrowptr")


def _pt10_structs(n=1000):
    z = np.load(os.path.join(G, "pt10_dataset.npz"))
    structs = [dict(positions=z["positions"][s], numbers=z["numbers"][s], cell=z["cell"][s], pbc=z["pbc"][s]) for s in range(n)]
    return structs, z["y"][:n], [str(v) for v in z["ids"][:n]]


def _both(structs, radius=8.0, k=12, dictionary=None):
    from matdeeplearn_amd.process import from_structures
    ys = np.zeros((len(structs), 1), dtype=np.float32)
    ids = [str(i) for i in range(len(structs))]
    host = from_structures(structs, ys, ids, radius, k, dictionary=dictionary)
    dev = from_structures(structs, ys, ids, radius, k, dictionary=dictionary, device="cuda")
    return host, dev


def _assert_bitwise(host, dev, what=""):
    for f in FIELDS:
        a, b = np.asarray(getattr(host, f)), np.asarray(getattr(dev, f))
        assert a.dtype == b.dtype and a.shape == b.shape, (what, f, a.dtype, b.dtype, a.shape, b.shape)
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), (what, f)
    assert host.dist_range == dev.dist_range, what


def _cloud(rng, n, grid=False, coincident=False):
    pos = rng.uniform(0.0, 9.0, size=(n, 3))
    if grid:                                                # lattice points: many exactly equal distances (rank ties)
        pos = np.round(pos / 1.5) * 1.5
    if coincident and n > 2:
        pos[1] = pos[0]
        pos[n - 1] = pos[0]
    return pos


def test_pt10_matches_reference_goldens_and_host_builder():
    from matdeeplearn_amd import ops
    from matdeeplearn_amd.process import from_structures
    from matdeeplearn_amd.process import graph as pg
    structs, ys, ids = _pt10_structs()
    gg = np.load(os.path.join(G, "pt10_graphs.npz"))
    host = from_structures(structs, ys, ids)
    dev = from_structures(structs, ys, ids, device="cuda")
    assert np.array_equal(np.diff(dev.edge_ptr), gg["edges_per_graph"]) and dev.num_edges == 99672
    for s in range(8):
        ei, ew, _ = pg.sort_by_target(gg["edge_index_%d" % s], gg["edge_weight_%d" % s])
        e0, e1 = dev.edge_ptr[s], dev.edge_ptr[s + 1]
        assert np.array_equal(dev.src[e0:e1], ei[0]) and np.array_equal(dev.tgt[e0:e1], ei[1])
        assert np.array_equal(dev.dist[e0:e1], ew)
    _assert_bitwise(host, dev, "pt10")
    # the op on its own, from tensors already on the device
    p = pg.pack_structures(structs)
    t = lambda a: torch.from_numpy(a).cuda()
    edge_ptr, src, tgt, dist, out_deg = ops.build_graphs(t(p["pos"]), t(p["node_ptr"]), t(p["cell"]), t(p["pbc"]), 8.0, 12)
    assert np.array_equal(edge_ptr.cpu().numpy(), host.edge_ptr) and np.array_equal(src.cpu().numpy(), host.src)
    assert np.array_equal(tgt.cpu().numpy(), host.tgt) and np.array_equal(dist.cpu().numpy(), host.dist)
    gl_src = host.src.astype(np.int64) + np.repeat(host.node_ptr[:-1], np.diff(host.edge_ptr))
    assert np.array_equal(out_deg.cpu().numpy(), np.bincount(gl_src, minlength=host.num_nodes))


@pytest.mark.parametrize("k", [1, 4, 12, 64])
@pytest.mark.parametrize("radius", [2.5, 4.0, 8.0])
def test_orthorhombic_and_open_clouds_every_pbc_bitwise(k, radius):
    rng = np.random.default_rng(1000 * k + int(radius * 10))
    structs = []
    for pbc_bits in range(8):
        pbc = [bool(pbc_bits >> a & 1) for a in range(3)]
        for grid in (False, True):
            for coincident in (False, True):
                n = int(rng.integers(1, 40))
                cell = np.diag(rng.uniform(5.0, 9.0, size=3))
                structs.append(dict(positions=_cloud(rng, n, grid, coincident), numbers=rng.integers(1, 90, size=n),
                                    cell=cell, pbc=np.array(pbc)))
    # one larger lattice cloud per call: ties across several 64-column chunks
    n = 150
    structs.append(dict(positions=np.round(rng.uniform(0, 12, size=(n, 3)) / 1.5) * 1.5, numbers=rng.integers(1, 90, size=n),
                        cell=np.diag([12.0, 12.0, 12.0]), pbc=np.array([True, True, True])))
    host, dev = _both(structs, radius, k)
    _assert_bitwise(host, dev, (k, radius))


def test_skewed_triclinic_cells_same_edges_distances_within_one_ulp():
    rng = np.random.default_rng(7)
    cells = [np.array([[4.0, 0, 0], [3.6, 1.2, 0], [0.3, 0.2, 9.0]]),
             np.array([[5.0, 0, 0], [9.0, 2.0, 0], [7.0, 5.0, 3.0]]),
             np.diag([6.0, 7.0, 8.0])]
    structs = []
    for cell in cells:
        for pbc in ([True, False, False], [False, True, False], [False, False, True], [True, True, False], [True, False, True],
                    [False, True, True], [True, True, True]):
            for n in (5, 30, 90):
                pos = rng.uniform(0, 1, size=(n, 3)) @ cell
                structs.append(dict(positions=pos, numbers=rng.integers(1, 90, size=n), cell=cell, pbc=np.array(pbc)))
    for k, radius in ((12, 8.0), (4, 4.0), (64, 8.0)):
        host, dev = _both(structs, radius, k)
        for f in ("node_ptr", "edge_ptr", "src", "tgt", "x", "z", "in_deg", "lrowptr"):
            assert np.array_equal(getattr(host, f), getattr(dev, f)), (k, radius, f)
        a, b = host.dist, dev.dist
        ulp = np.spacing(np.maximum(np.abs(a), np.abs(b)))
        assert np.all(np.abs(a - b) <= ulp), (k, radius, np.abs(a - b).max())


def test_sizes_single_atoms_isolated_atoms_large_and_mixed_graphs():
    rng = np.random.default_rng(3)
    structs = [dict(positions=np.zeros((1, 3)), numbers=np.array([6]), cell=np.eye(3) * 5.0, pbc=np.array([True] * 3)),
               dict(positions=np.array([[0.0, 0, 0]]), numbers=np.array([1]), cell=None, pbc=None),
               # atoms 50 A apart: no neighbour within the radius
               dict(positions=np.arange(5)[:, None] * np.array([[50.0, 0, 0]]), numbers=np.arange(1, 6), cell=np.zeros((3, 3)),
                    pbc=np.array([False] * 3))]
    host, dev = _both(structs)
    _assert_bitwise(host, dev, "tiny")
    assert np.array_equal(np.diff(dev.edge_ptr), [1, 1, 5])
    # one graph of 2048 atoms (32 column chunks per row)
    n = 2048
    big = [dict(positions=rng.uniform(0, 30.0, size=(n, 3)), numbers=rng.integers(1, 90, size=n), cell=np.diag([30.0] * 3),
                pbc=np.array([True] * 3))]
    host, dev = _both(big)
    _assert_bitwise(host, dev, "2048")
    # mixed 1..500 atoms: across the 64-column chunks and the 2048-node scan tiles
    sizes = np.concatenate([[1, 2, 63, 64, 65, 127, 128, 129, 500], rng.integers(1, 501, size=30)])
    mixed = []
    for i, n in enumerate(sizes):
        side = (n / 0.05) ** (1 / 3)
        mixed.append(dict(positions=rng.uniform(0, side, size=(n, 3)), numbers=rng.integers(1, 90, size=n),
                          cell=np.diag([side] * 3), pbc=np.array([i % 3 != 0] * 3)))
    host, dev = _both(mixed)
    assert dev.num_nodes > 2 * 2048
    _assert_bitwise(host, dev, "mixed")


def test_dictionary_features_determinism_and_argument_errors():
    from matdeeplearn_amd import ops
    from matdeeplearn_amd.process import from_structures
    from matdeeplearn_amd.process import graph as pg
    structs, ys, ids = _pt10_structs(60)
    rng = np.random.default_rng(0)
    table = {str(z): list(rng.normal(size=9).astype(np.float32).astype(float)) for z in range(1, 101)}
    host, dev = _both(structs, dictionary=table)
    _assert_bitwise(host, dev, "dictionary")
    assert dev.x.shape[1] == 9 + 14
    # run to run: bitwise the same
    a = from_structures(structs, ys, ids, device="cuda")
    b = from_structures(structs, ys, ids, device="cuda")
    _assert_bitwise(a, b, "rerun")
    p = pg.pack_structures(structs)
    t = lambda v: torch.from_numpy(v).cuda()
    args = (t(p["pos"]), t(p["node_ptr"]), t(p["cell"]), t(p["pbc"]))
    for k in (0, 65):
        with pytest.raises(ops.MdlError):
            ops.build_graphs(*args, 8.0, k)
    for r in (0.0, -1.0):
        with pytest.raises(ops.MdlError):
            ops.build_graphs(*args, r, 12)
    bad = p["node_ptr"].copy()
    bad[3], bad[4] = bad[4], bad[3]
    with pytest.raises(ops.MdlError):
        ops.build_graphs(args[0], t(bad), args[2], args[3], 8.0, 12)
    with pytest.raises(ops.MdlError):
        ops.build_graphs(args[0].float(), *args[1:], 8.0, 12)


def test_one_epoch_on_device_built_pt10_equals_host_built():
    from matdeeplearn_amd import ops
    from matdeeplearn_amd.process import from_structures
    from matdeeplearn_amd.training import train_regular
    structs, ys, ids = _pt10_structs()
    training = dict(target_index=0, loss="l1_loss", train_ratio=0.8, val_ratio=0.1, test_ratio=0.1, verbosity=0)
    mp = dict(model="CGCNN", dim1=32, dim2=32, pre_fc_count=1, gc_count=2, post_fc_count=1, epochs=1, lr=0.002,
              batch_size=100, optimizer="AdamW", optimizer_args={}, scheduler="ReduceLROnPlateau",
              scheduler_args={"mode": "min", "factor": 0.8, "patience": 10}, batch_norm="False")
    job = dict(job_name="g", seed=5, save_model="False", write_output="False")
    quiet = lambda *a: None
    prev = ops.configure(deterministic=True)
    try:
        runs = []
        for device in (None, "cuda"):
            ds = from_structures(structs, ys, ids, device=device).to("cuda")
            runs.append(train_regular("cuda", 1, ds, job, dict(training, graph_replay="False"), mp, log=quiet))
    finally:
        ops.configure(**prev)
    h, d = runs[0]["history"], runs[1]["history"]
    assert h[0]["edges"] == d[0]["edges"] > 0
    assert [x["train"] for x in h] == [x["train"] for x in d]
    assert runs[0]["val_error"] == runs[1]["val_error"]
