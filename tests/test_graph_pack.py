"""CPU: graph.pack_structures, the host half of the device graph builder (process.from_structures(device=...)) — flat
positions / numbers, node_ptr, per-structure cells and the pbc bitmask from mixed structure dicts — and the argument checks
that need no device."""
import numpy as np
import pytest
import torch


def test_pack_structures_mixed_inputs():
    from matdeeplearn_amd.process import graph as pg
    rng = np.random.default_rng(0)
    cell = np.array([[4.0, 0, 0], [3.6, 1.2, 0], [0.3, 0.2, 9.0]])
    structs = [dict(positions=rng.normal(size=(3, 3)), numbers=[1, 6, 8], cell=cell, pbc=np.array([True, False, True])),
               dict(positions=rng.normal(size=(1, 3)).tolist(), numbers=np.array([26]), cell=None, pbc=None),
               dict(positions=np.zeros((0, 3)), numbers=np.zeros(0, dtype=np.int64), cell=np.eye(3).ravel(), pbc=True),
               dict(positions=rng.normal(size=(4, 3)).astype(np.float32), numbers=np.array([1, 1, 2, 3], dtype=np.int32),
                    pbc=[False, True, False])]
    p = pg.pack_structures(iter(structs))
    assert p["node_ptr"].dtype == np.int64 and p["node_ptr"].tolist() == [0, 3, 4, 4, 8]
    assert p["pos"].dtype == np.float64 and p["pos"].shape == (8, 3)
    assert np.array_equal(p["pos"][:3], structs[0]["positions"]) and np.array_equal(p["pos"][3], structs[1]["positions"][0])
    assert np.array_equal(p["pos"][4:], structs[3]["positions"].astype(np.float64))
    assert p["numbers"].dtype == np.int64 and p["numbers"].tolist() == [1, 6, 8, 26, 1, 1, 2, 3]
    assert p["cell"].dtype == np.float64 and p["cell"].shape == (4, 3, 3)
    assert np.array_equal(p["cell"][0], cell) and not p["cell"][1].any() and np.array_equal(p["cell"][2], np.eye(3))
    assert not p["cell"][3].any()
    assert p["pbc"].dtype == np.int32 and p["pbc"].tolist() == [0b101, 0, 0b111, 0b010]
    with pytest.raises(ValueError):
        pg.pack_structures([])


def test_from_structures_device_path_needs_a_hip_device():
    from matdeeplearn_amd import ops
    from matdeeplearn_amd.process import from_structures
    structs = [dict(positions=np.zeros((2, 3)), numbers=[1, 1], cell=None, pbc=None)]
    with pytest.raises(ops.MdlError):
        ops.build_graphs(torch.zeros(2, 3, dtype=torch.float64), torch.tensor([0, 2]), torch.zeros(1, 3, 3, dtype=torch.float64),
                         torch.zeros(1, dtype=torch.int32))
    if not torch.cuda.is_available():
        with pytest.raises(Exception):
            from_structures(structs, np.zeros((1, 1)), ["a"], device="cuda")
