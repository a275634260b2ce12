"""GPU checks of molecular dynamics at constant pressure: the cell mode of mdl_md_step (csrc/md.hip, ops.md_cell_step) against
md_cell_reference, the fp64 restatement that tests/test_md_cell_host.py owns — every branch in one launch, the structures without a
barostat to the bit of ops.md_step, the same bits from the same inputs, alone and in a batch —, the ideal-gas test of the host file
through the device, and forces.md_npt against the fp64 trajectory of the oracle CGCNN at held neighbour lists (bounds:
NPT_TRAJ_BOUND_POS and NPT_TRAJ_BOUND_CELL of the host file).

Figures measured on the MI355X are in the docstrings of the tests."""
import math

import numpy as np
import pytest
import torch

import test_gpu_md as tgm
import test_md_cell_host as tch
import test_md_host as tmh
import test_relax_host as trh
from test_gpu_forces import DIST_RANGE, dev

pytestmark = pytest.mark.gpu

# the 13 roles of test_gpu_md without a barostat, then the barostat's: one atom, a pair, a wave - 1, exactly one wave, a wave + 1, a
# pass of 256 + 1, two passes + 1, empty, and what the other roles need
N_PLAIN = len(tgm.SIZES)
BARO_SIZES = [1, 2, 63, 64, 65, 33, 0, 40, 17, 257, 513, 70, 30]
(B_FIRST, B_LATER, B_LANGEVIN, B_COLD, B_SOME_FIXED, B_ALL_FIXED, B_EMPTY, B_CLOSING, B_STOPPED, B_GUARD_DISP, B_GUARD_STRAIN, B_NAN_S,
 B_NO_VOLUME) = range(N_PLAIN, N_PLAIN + 13)
SIZES = tgm.SIZES + BARO_SIZES
MAX_DISP, MAX_STRAIN = tgm.MAX_DISP, 0.1
STATE_KEYS = ("steps", "status", "ekin", "volume", "pressure")


def _cell_inputs():
    """test_gpu_md._md_inputs with rate = 0, followed by seeded structures that put every branch of the barostat into the same
    launch (the roles above, by structure).  Returns the arguments of md_cell_reference, max_disp and max_strain left out."""
    ppos, pvel, pforce, pmass, pptr, pst, pdt, pn_steps, pgamma, pkT, pseed, pfixed = tgm._md_inputs()
    rng = np.random.default_rng(23)
    nb, n_new = len(BARO_SIZES), int(np.sum(BARO_SIZES))
    node_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    B = len(SIZES)
    seg = lambda b: slice(node_ptr[b] - node_ptr[N_PLAIN], node_ptr[b + 1] - node_ptr[N_PLAIN])      # rows of the new arrays
    force = rng.normal(size=(n_new, 3)).astype(np.float32)
    vel = 0.3 * rng.normal(size=(n_new, 3))
    pos = rng.uniform(0.0, 9.0, (n_new, 3))
    mass = rng.uniform(1.0, 20.0, n_new)
    fixed = np.zeros(n_new, np.uint8)
    fixed[seg(B_ALL_FIXED)] = 1
    fixed[seg(B_SOME_FIXED)][::4] = 1
    st = tch.new_cell_state(B)
    st["steps"] = np.concatenate([pst["steps"], np.array([0, 9, 5, 3, 7, 2, 4, 25, 6, 0, 8, 1, 2], np.int32)])
    st["status"][:N_PLAIN] = pst["status"]
    st["status"][B_STOPPED] = 3
    st["ekin"][:], st["volume"][:], st["pressure"][:] = -1.0, -2.0, -3.0
    n_steps = np.concatenate([pn_steps, np.full(nb, 2 ** 21, np.int32)])
    n_steps[B_CLOSING] = 25
    dt = np.concatenate([pdt, rng.uniform(0.05, 0.15, nb)])
    gamma = np.concatenate([pgamma, np.zeros(nb)])
    for b in (B_LANGEVIN, B_COLD, B_SOME_FIXED, B_CLOSING, B_STOPPED, B_GUARD_DISP, B_NO_VOLUME):
        gamma[b] = rng.uniform(1.0, 8.0)
    kT = np.concatenate([pkT, rng.uniform(0.2, 1.0, nb)])
    kT[B_COLD] = 0.0
    seed = np.concatenate([pseed, rng.integers(-2 ** 62, 2 ** 62, nb)])
    cell, S = tch.cells_for(B, seed=29)
    cell[B_NO_VOLUME, 2] = 0.0                                    # a cell without a third lattice vector: det = 0 exactly
    S[B_NAN_S, 1, 1] = np.nan
    pressure = rng.uniform(-0.02, 0.02, B)
    rate = np.concatenate([np.zeros(N_PLAIN), rng.uniform(2.0, 6.0, nb)])
    pressure[B_GUARD_STRAIN] = 40.0                              # d eps = -rate (P0 - P_int) dt: of order -4 to -36
    force[seg(B_GUARD_DISP)][11] = [3e5, -2e5, 1e5]                # finite, and far too large a step; at steps == 0 no kick has put it into ekin
    cat = lambda a, b: np.concatenate([a, b])
    return (cat(ppos, pos), cat(pvel, vel), cell, cat(pforce, force), S, cat(pmass, mass), node_ptr, st, dt, n_steps, pressure, rate, gamma, kT,
            seed, cat(pfixed, fixed))


def _to_dev(pos, vel, cell, force, S, mass, node_ptr, st, dt, n_steps, pressure, rate, gamma, kT, seed, fixed):
    from matdeeplearn_amd import ops
    d = dev()
    t = lambda a: torch.from_numpy(np.array(a)).to(d)
    state = ops.MDCellState(*[t(st[k]) for k in STATE_KEYS])
    return [t(pos), t(vel), t(cell), t(force), t(S), t(mass), t(node_ptr), state, t(dt), t(n_steps), t(pressure), t(rate), t(gamma), t(kT),
            t(seed), t(fixed)]


def _launch(inp):
    from matdeeplearn_amd import ops
    a = _to_dev(*inp)
    out = ops.md_cell_step(*a, max_disp=MAX_DISP, max_strain=MAX_STRAIN)
    assert out is a[7]
    return a[0], a[1], a[2], a[7]


def _close_nan(got, ref, name):
    """[B] values: NaN where the reference has one, else tgm._close's bound"""
    g = got.cpu().numpy()
    assert np.array_equal(np.isnan(g), np.isnan(ref)), (name, g, ref)
    tgm._close(torch.from_numpy(np.nan_to_num(g)), np.nan_to_num(ref), np.arange(len(ref) + 1), name)


def test_md_cell_step_matches_the_host_reference_in_every_branch():
    """On the MI355X: pos 8.9e-17, vel 4.4e-16, ekin 3.0e-16, pressure 2.8e-16 of a structure's largest magnitude at worst; cell and
    volume carry the reference's bits."""
    from matdeeplearn_amd import ops
    inp = _cell_inputs()
    pos, vel, cell, force, S, mass, node_ptr, st, dt, n_steps, pressure, rate, gamma, kT, seed, fixed = inp
    B = len(SIZES)
    assert {0, 1, 2, 63, 64, 65, 257, 513} <= set(BARO_SIZES)
    rpos, rvel, rcell, rst, diag = tch.md_cell_reference(*inp, max_disp=MAX_DISP, max_strain=MAX_STRAIN)
    # the reference's own values: every branch is there, and no decision is marginal
    want = {B_FIRST: "nve", B_LATER: "nve", B_LANGEVIN: "langevin", B_COLD: "langevin", B_SOME_FIXED: "langevin", B_ALL_FIXED: "nve",
            B_EMPTY: "nve", B_CLOSING: "closing", B_STOPPED: "stopped", B_GUARD_DISP: "refused", B_GUARD_STRAIN: "strained",
            B_NAN_S: "strained", B_NO_VOLUME: "strained"}
    assert {b: diag[b]["branch"] for b in want} == want
    assert [d["branch"] for d in diag[:N_PLAIN]] == [d["branch"] for d in tmh.md_reference(*tgm._md_inputs(), max_disp=MAX_DISP)[3]]
    assert st["steps"][B_FIRST] == 0 and st["steps"][B_LATER] > 0 and kT[B_COLD] == 0 and kT[B_LANGEVIN] > 0
    for b in range(B):
        disp, deps = diag[b]["disp"], diag[b]["deps"]
        assert (np.isnan(disp) | (np.abs(disp - MAX_DISP) >= 1e-3)).all(), (b, disp)
        assert diag[b]["baro"] == (b >= N_PLAIN and b not in (B_CLOSING, B_STOPPED)), b
        assert not diag[b]["baro"] or np.isnan(deps) or abs(abs(deps) - MAX_STRAIN) >= 1e-3, (b, deps)
    accepted_baro = (B_FIRST, B_LATER, B_LANGEVIN, B_COLD, B_SOME_FIXED, B_ALL_FIXED, B_EMPTY)
    assert all(1e-4 < abs(diag[b]["deps"]) < MAX_STRAIN for b in accepted_baro + (B_GUARD_DISP,)), [diag[b]["deps"] for b in accepted_baro]
    assert np.isfinite(diag[B_GUARD_STRAIN]["deps"]) and abs(diag[B_GUARD_STRAIN]["deps"]) > 1.0 and np.isnan(diag[B_NAN_S]["deps"])
    assert diag[B_NO_VOLUME]["volume"] == 0.0 and (diag[B_GUARD_DISP]["disp"] > MAX_DISP).sum() == 1

    dpos, dvel, dcell, state = _launch(inp)
    for k in ("steps", "status"):
        assert np.array_equal(getattr(state, k).cpu().numpy(), rst[k]), (k, getattr(state, k), rst[k])
    assert state.status.cpu().tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2] + [0, 0, 0, 0, 0, 0, 0, 1, 3, 2, 3, 3, 3]
    tgm._close(dpos, rpos, node_ptr, "pos")
    tgm._close(dvel, rvel, node_ptr, "vel")
    tgm._close(dcell.reshape(-1, 3), rcell.reshape(-1, 3), 3 * np.arange(B + 1), "cell")
    for k in ("ekin", "volume", "pressure"):
        _close_nan(getattr(state, k), rst[k], k)
    gpos, gvel, gcell = dpos.cpu().numpy(), dvel.cpu().numpy(), dcell.cpu().numpy()
    seg = lambda b: slice(node_ptr[b], node_ptr[b + 1])
    # without a barostat: the bits of ops.md_step on the same inputs, and the cell is not written
    a = tgm._to_dev(*tgm._md_inputs())
    ops.md_step(*a, max_disp=MAX_DISP)
    n_plain = int(node_ptr[N_PLAIN])
    assert torch.equal(dpos[:n_plain], a[0]) and torch.equal(dvel[:n_plain], a[1])
    for k in ("steps", "status", "ekin"):
        assert torch.equal(getattr(state, k)[:N_PLAIN], getattr(a[5], k)), k
    assert np.array_equal(gcell[:N_PLAIN], cell[:N_PLAIN])
    # stopped before: every bit is what went in; volume and pressure of a running structure are written whatever it does next
    for b in (tgm.FINISHED, tgm.REFUSED_BEFORE, B_STOPPED):
        assert np.array_equal(gpos[seg(b)], pos[seg(b)]) and np.array_equal(gvel[seg(b)], vel[seg(b)]) and np.array_equal(gcell[b], cell[b])
        assert [float(getattr(state, k)[b]) for k in ("ekin", "volume", "pressure")] == [-1.0, -2.0, -3.0]
    written = [b for b in range(B) if b not in (tgm.FINISHED, tgm.REFUSED_BEFORE, B_STOPPED)]
    assert all(float(state.volume[b]) != -2.0 and float(state.pressure[b]) != -3.0 for b in written)
    assert math.isnan(float(state.volume[B_NO_VOLUME])) and math.isnan(float(state.pressure[B_NO_VOLUME]))
    assert math.isnan(float(state.pressure[B_NAN_S])) and float(state.volume[B_NAN_S]) > 0
    # closing and every refusal: positions and cell keep their bits
    for b in (B_CLOSING, B_GUARD_DISP, B_GUARD_STRAIN, B_NAN_S, B_NO_VOLUME):
        assert np.array_equal(gpos[seg(b)], pos[seg(b)]) and np.array_equal(gcell[b], cell[b]), b
    assert np.isfinite(gpos).all() and np.isfinite(gvel).all() and np.isfinite(gcell).all()
    # accepted with a barostat: the cell is the old one times s = exp(d eps / 3); fixed atoms ride with it and have no velocity
    for b in accepted_baro:
        s = np.exp(diag[b]["deps"] / 3.0)
        assert np.abs(gcell[b] - s * cell[b]).max() <= 1e-12 * np.abs(cell[b]).max() and not np.array_equal(gcell[b], cell[b]), b
        fx = fixed[seg(b)] != 0
        assert np.abs(gpos[seg(b)][fx] - s * pos[seg(b)][fx]).max(initial=0.0) <= 1e-12 * 9.0 and not gvel[seg(b)][fx].any()
        assert (gpos[seg(b)] != pos[seg(b)]).any(1).all()
    assert float(state.ekin[B_ALL_FIXED]) == 0.0 and float(state.ekin[B_EMPTY]) == 0.0 and int(state.steps[B_EMPTY]) == st["steps"][B_EMPTY] + 1


def test_md_cell_step_repeats_its_bits_alone_and_in_any_batch():
    inp = _cell_inputs()
    pos, vel, cell, force, S, mass, node_ptr, st, dt, n_steps, pressure, rate, gamma, kT, seed, fixed = inp
    first, second = _launch(inp), _launch(inp)
    for a, b in zip(first[:3], second[:3]):
        assert torch.equal(a, b)
    eq = lambda a, b: torch.equal(a, b) or (torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a), torch.nan_to_num(b)))
    for k in STATE_KEYS:
        assert eq(getattr(first[3], k), getattr(second[3], k)), k
    dpos, dvel, dcell, state = first
    for b in range(len(SIZES)):                                   # each structure alone, with its key
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        one = {k: v[b:b + 1] for k, v in st.items()}
        alone = (pos[a:e], vel[a:e], cell[b:b + 1], force[a:e], S[b:b + 1], mass[a:e], np.array([0, e - a]), one, dt[b:b + 1], n_steps[b:b + 1],
                 pressure[b:b + 1], rate[b:b + 1], gamma[b:b + 1], kT[b:b + 1], seed[b:b + 1], fixed[a:e])
        apos, avel, acell, astate = _launch(alone)
        assert torch.equal(apos, dpos[a:e]) and torch.equal(avel, dvel[a:e]), b
        for k in STATE_KEYS if e > a else ():                    # (N == 0 is no launch by the C ABI: an empty batch has no barostat)
            assert eq(getattr(astate, k), getattr(state, k)[b:b + 1]), (b, k)
        assert e == a or torch.equal(acell[0], dcell[b]), b
    # kT = 0 draws no number: another seed, the same bits; with kT > 0 the barostat's noise moves the cell elsewhere
    arg = list(inp)
    arg[14] = seed + 1
    other = _launch(arg)
    assert torch.equal(other[2][B_COLD], dcell[B_COLD]) and torch.equal(other[0][node_ptr[B_COLD]:node_ptr[B_COLD + 1]], dpos[node_ptr[B_COLD]:node_ptr[B_COLD + 1]])
    assert not torch.equal(other[2][B_FIRST], dcell[B_FIRST]) and not torch.equal(other[2][B_EMPTY], dcell[B_EMPTY])


def test_md_cell_step_rejects_bad_arguments_on_the_device():
    from matdeeplearn_amd import ops
    names = ("pos", "vel", "cell", "force", "strain_grad", "mass", "node_ptr", "state", "dt", "n_steps", "pressure", "rate", "gamma", "kT", "seed",
             "fixed")
    args = dict(zip(names, _to_dev(*_cell_inputs())))

    def bad(**kw):
        a = dict(args, **kw)
        with pytest.raises(ops.MdlError):
            ops.md_cell_step(*[a[k] for k in names], a.get("max_disp", MAX_DISP), a.get("max_strain", MAX_STRAIN))

    bad(cell=args["cell"].float())
    bad(cell=args["cell"][:-1])
    bad(cell=args["cell"].transpose(1, 2))                                  # not contiguous: the update is in place
    bad(cell=args["cell"].cpu())
    bad(strain_grad=args["strain_grad"].double())
    bad(strain_grad=args["strain_grad"][:-1])
    bad(rate=-args["rate"] - 1.0)
    bad(rate=args["rate"].float())
    bad(pressure=args["pressure"][:-1])
    bad(state=ops.md_state(len(SIZES), dev()))
    bad(state=ops.md_cell_state(len(SIZES) - 1, dev()))
    bad(max_strain=0.0)
    bad(max_strain=float("nan"))
    ref = _to_dev(*_cell_inputs())
    assert torch.equal(args["pos"], ref[0]) and torch.equal(args["cell"], ref[2]) and torch.equal(args["state"].steps, ref[7].steps)
    fresh = ops.md_cell_state(3, dev())
    assert torch.isnan(fresh.volume).all() and torch.isnan(fresh.pressure).all() and not fresh.status.any() and fresh.volume.dtype == torch.float64
    # the C ABI: in the cell mode every cell-mode pointer must be there and max_strain > 0
    from matdeeplearn_amd._lib import lib, ptr, stream
    a = [args[k] for k in names]
    per = ops._md_per_structure("md_cell_step", (("dt", a[8]), ("gamma", a[12]), ("kT", a[13]), ("seed", a[14]), ("n_steps", a[9])), len(SIZES), dev(), {})
    head = [ptr(a[0]), ptr(a[1]), ptr(a[3]), ptr(a[5]), ptr(a[15]), ptr(a[6]), a[0].shape[0], len(SIZES)] + [ptr(t) for t in per] + [
        ptr(a[7].steps), ptr(a[7].status), ptr(a[7].ekin), MAX_DISP]
    cellm = [ptr(a[2]), ptr(a[4]), ptr(a[10]), ptr(a[11]), ptr(a[7].volume), ptr(a[7].pressure)]
    for k in range(1, 6):
        assert lib().mdl_md_step(*head, *(cellm[:k] + [None] + cellm[k + 1:]), MAX_STRAIN, stream()) != 0, k
    assert lib().mdl_md_step(*head, *cellm, 0.0, stream()) != 0
    torch.cuda.synchronize()
    assert torch.equal(args["pos"], ref[0]) and torch.equal(args["cell"], ref[2])


def test_ideal_gas_keeps_its_equation_of_state_on_the_device():
    """tests/test_md_cell_host.py's ideal gas through ops.md_cell_step: 64 structures of 32 atoms, 1501 launches.  On the MI355X:
    <V> / 462 - 1 = -9.2e-3 with SE 6.1e-3 (1.52 SE); the device volumes leave the host trajectory by 5.3e-15 (relative) at most — a figure, not
    a bound: without forces nothing amplifies a rounding difference."""
    from matdeeplearn_amd import ops
    g = tch.IDEAL_GAS
    pos, vel, cell, mass, node_ptr = tch.ideal_gas_case()
    d, B = dev(), g["structures"]
    t = lambda a: torch.from_numpy(np.array(a)).to(d)
    dpos, dvel, dcell, dmass, dptr, state = t(pos), t(vel), t(cell), t(mass), t(node_ptr), ops.md_cell_state(B, d)
    force, S = torch.zeros(len(pos), 3, device=d), torch.zeros(B, 3, 3, device=d)
    n_steps = torch.full((B,), g["steps"], dtype=torch.int32, device=d)
    volumes = torch.empty(g["steps"] + 1, B, dtype=torch.float64, device=d)
    for it in range(g["steps"] + 1):
        ops.md_cell_step(dpos, dvel, dcell, force, S, dmass, dptr, state, g["dt"], n_steps, g["pressure"], g["rate"], g["gamma"], g["kT"], g["seed"],
                         max_disp=1e9, max_strain=g["max_strain"])
        volumes[it].copy_(state.volume)
    assert (state.status == 1).all() and (state.steps == g["steps"]).all()
    got = volumes.cpu().numpy()
    tch.ideal_gas_check(got)
    ref = tch.ideal_gas_reference()[0]
    print("device volumes against the host trajectory: largest relative difference %.3e" % np.abs(got / ref - 1.0).max())


# ---------------------------------------------------------------------------------------------
# forces.md_npt
# ---------------------------------------------------------------------------------------------
def _npt(model, case, **kw):
    from matdeeplearn_amd import forces
    a = tch.NPT_ARGS
    args = dict(dt=a["dt"], steps=a["steps"], pressure=a["pressure"], tau_p=1.0, compressibility=a["rate"], kT=a["kT"], seed=a["seed"],
                max_strain=a["max_strain"], velocities=tmh.md_initial_velocities(case), rebuild_every=0)
    args.update(kw)
    return forces.md_npt(model, case.structs, DIST_RANGE, tmh.md_masses(case), **args)


def test_md_npt_follows_the_fp64_reference_trajectory_at_held_lists():
    """On the MI355X: the final positions are 1.4e-7 A and the final lattice vectors 1.2e-8 A from the fp64 trajectory (bounds 2.7e-4
    and 6.6e-6 A), the volumes 7.1e-9 (relative) at most along the way; they shrink by 2.2 % to 11.4 %."""
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    ref_pos, ref_vel, ref_cell, ref_vol, _, _ = tch.cgcnn_npt_reference()
    model, B, N, steps = tgm._oracle_model(), len(case.structs), len(case.p["pos"]), tch.NPT_ARGS["steps"]
    with ops.deterministic():
        res = _npt(model, case)
        again = _npt(model, case)
        other = _npt(model, case, seed=tch.NPT_ARGS["seed"] + 1)
        ff = forces.ForceField(model, case.structs, DIST_RANGE)             # the lists of the initial geometry
        ff.set_positions(res.positions)
        ff.set_cell(res.cell)
        e_held, f_held = ff.evaluate()
    assert isinstance(res, forces.NPTResult)
    for k in ("positions", "velocities", "cell", "ekin", "volume", "pressure", "ekin_trace", "volume_trace", "pressure_trace"):
        assert getattr(res, k).dtype == torch.float64, k
    assert res.steps.dtype == torch.int32 and res.status.dtype == torch.int32 and res.forces.dtype == torch.float32 and res.energy.dtype == torch.float32
    assert tuple(res.positions.shape) == (N, 3) == tuple(res.velocities.shape) == tuple(res.forces.shape) and tuple(res.cell.shape) == (B, 3, 3)
    assert all(tuple(getattr(res, k).shape) == (B,) for k in ("energy", "ekin", "volume", "pressure", "steps", "status"))
    assert all(tuple(getattr(res, k).shape) == (steps + 1, B) for k in ("epot_trace", "ekin_trace", "volume_trace", "pressure_trace"))
    assert (res.steps == steps).all() and (res.status == 1).all() and not any(torch.isnan(getattr(res, k)).any() for k in res._fields[:-1] if getattr(res, k).is_floating_point())
    assert torch.equal(res.energy, e_held) and torch.equal(res.forces, f_held) and torch.equal(res.epot_trace[-1], res.energy)
    assert torch.equal(res.volume_trace[-1], res.volume) and torch.equal(res.pressure_trace[-1], res.pressure) and torch.equal(res.ekin_trace[-1], res.ekin)
    for a, b in zip(res, again):
        assert torch.equal(a, b)
    assert not torch.equal(res.cell, other.cell) and not torch.equal(res.positions, other.positions)       # the barostat's noise is on
    dev_pos = np.sqrt(((res.positions.cpu().numpy() - ref_pos) ** 2).sum(1)).max()
    dev_cell = np.sqrt(((res.cell.cpu().numpy() - ref_cell) ** 2).sum(2)).max()
    vol = res.volume_trace.cpu().numpy()
    print("largest distance from the reference trajectory: positions %.3e A (bound %.1e), lattice vectors %.3e A (bound %.1e)"
          % (dev_pos, tch.NPT_TRAJ_BOUND_POS, dev_cell, tch.NPT_TRAJ_BOUND_CELL))
    print("relative volume change", vol[-1] / vol[0] - 1.0, "volumes against the reference %.3e (relative)" % np.abs(vol / ref_vol - 1.0).max())
    print("velocities: largest difference %.3e of %.3e" % (np.abs(res.velocities.cpu().numpy() - ref_vel).max(), np.abs(ref_vel).max()))
    assert (np.abs(vol[-1] / vol[0] - 1.0) >= 0.01).all()
    assert dev_pos <= tch.NPT_TRAJ_BOUND_POS and dev_cell <= tch.NPT_TRAJ_BOUND_CELL
    det = torch.linalg.det(res.cell).abs()
    assert torch.allclose(det, res.volume, rtol=1e-12, atol=0.0)


def test_md_npt_without_a_barostat_is_md_and_its_strain_guard_stops_where_it_started():
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    model, masses, B = tgm._oracle_model(), tmh.md_masses(case), len(case.structs)
    node_ptr = case.p["node_ptr"]
    args = dict(dt=1.0, steps=6, kT=2e-5, gamma=0.05, seed=3, rebuild_every=0)
    tau = np.full(B, 1.0)
    tau[2] = math.inf
    with ops.deterministic():
        plain = forces.md(model, case.structs, DIST_RANGE, masses, **args)                          # held lists, velocities drawn
        npt = forces.md_npt(model, case.structs, DIST_RANGE, masses, pressure=3e-5, tau_p=tau, compressibility=30.0, **args)
    a, e = int(node_ptr[2]), int(node_ptr[3])
    assert torch.equal(npt.positions[a:e], plain.positions[a:e]) and torch.equal(npt.velocities[a:e], plain.velocities[a:e])
    assert torch.equal(npt.ekin_trace[:, 2], plain.ekin_trace[:, 2]) and torch.equal(npt.epot_trace[:, 2], plain.epot_trace[:, 2])
    assert torch.equal(npt.forces[a:e], plain.forces[a:e]) and np.array_equal(npt.cell[2].cpu().numpy(), case.p["cell"][2])
    assert (npt.status == 1).all() and (npt.steps == 6).all()
    others = [b for b in range(B) if b != 2]
    assert all(not np.array_equal(npt.cell[b].cpu().numpy(), case.p["cell"][b]) for b in others)
    assert not torch.equal(npt.positions[:a], plain.positions[:a])
    assert torch.isfinite(npt.volume).all() and torch.isfinite(npt.pressure).all()
    # a max_strain below the first step stops every barostatted structure with status 3 at its starting geometry
    stopped = forces.md_npt(model, case.structs, DIST_RANGE, masses, pressure=3e-5, tau_p=tau, compressibility=30.0, max_strain=1e-12,
                            check_every=1, **args)
    assert stopped.status.cpu().tolist() == [3, 3, 1, 3, 3, 3] and stopped.steps.cpu().tolist() == [0, 0, 6, 0, 0, 0]
    pos, cell = stopped.positions.cpu().numpy(), stopped.cell.cpu().numpy()
    keep = np.ones(len(pos), bool)
    keep[a:e] = False
    assert np.array_equal(pos[keep], case.p["pos"][keep]) and np.array_equal(cell, case.p["cell"])
    assert not torch.isnan(stopped.volume_trace[0]).any()
