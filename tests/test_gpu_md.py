"""GPU checks of the molecular-dynamics path: the batched BAOAB update and the Maxwell-Boltzmann draw of csrc/md.hip (ops.md_step,
ops.md_velocities) against the fp64 restatements that tests/test_md_host.py owns — every branch in one launch, the same bits from
the same inputs, alone and in a batch —, the Langevin sampling test of the host file through the device, and forces.md against the
fp64 trajectory of the oracle CGCNN at held neighbour lists (bounds: MD_TRAJ_BOUND and MD_ENERGY_EXCURSION of the host file).

Figures measured on the MI355X are in the docstrings of the tests."""
import numpy as np
import pytest
import torch

import test_gpu_forces as tgf
import test_md_host as tmh
import test_relax_host as trh
from test_gpu_forces import DIST_RANGE, DS, dev

pytestmark = pytest.mark.gpu

# one atom, a pair, a wave - 1, exactly one wave, a wave + 1, empty, a pass of 256 + 1, two passes + 1, and what the other roles need
SIZES = [1, 2, 63, 64, 65, 0, 257, 513, 33, 40, 70, 300, 17]
FIRST, NVE, LANGEVIN, COLD, SOME_FIXED, EMPTY, ALL_FIXED, LATER, CLOSING, FINISHED, GUARD_BIG, GUARD_NAN, REFUSED_BEFORE = range(13)
MAX_DISP = 0.5


def _md_inputs():
    """seeded inputs that put every branch of the update into one launch (the roles above, by structure)"""
    rng = np.random.default_rng(17)
    node_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    N, B = int(node_ptr[-1]), len(SIZES)
    seg = lambda b: slice(node_ptr[b], node_ptr[b + 1])
    force = rng.normal(size=(N, 3)).astype(np.float32)
    vel = 0.3 * rng.normal(size=(N, 3))
    pos = rng.uniform(0.0, 10.0, (N, 3))
    mass = rng.uniform(1.0, 20.0, N)
    fixed = np.zeros(N, np.uint8)
    fixed[seg(ALL_FIXED)] = 1
    fixed[seg(SOME_FIXED)][::4] = 1
    fixed[seg(LATER)][5::9] = 1
    st = tmh.new_state(B)
    st["steps"] = np.array([0, 3, 0, 12, 7, 2, 4, 2 ** 20, 25, 25, 3, 0, 6], np.int32)
    st["status"][FINISHED], st["status"][REFUSED_BEFORE] = 1, 2
    st["ekin"][:] = -1.0
    n_steps = np.full(B, 2 ** 21, np.int32)
    n_steps[CLOSING] = n_steps[FINISHED] = 25
    dt = rng.uniform(0.05, 0.15, B)
    gamma = np.zeros(B)
    for b in (LANGEVIN, COLD, SOME_FIXED, LATER, CLOSING, FINISHED, GUARD_BIG, REFUSED_BEFORE):
        gamma[b] = rng.uniform(1.0, 8.0)
    kT = rng.uniform(0.2, 1.0, B)
    kT[COLD] = 0.0
    seed = rng.integers(-2 ** 62, 2 ** 62, B)                      # both halves of the key in use, either sign
    seed[LANGEVIN], seed[LATER] = 5, -1
    force[seg(GUARD_BIG)][11] = [3e5, -2e5, 1e5]                   # finite, and far too large a step
    force[seg(GUARD_NAN)][123, 1] = np.nan
    return pos, vel, force, mass, node_ptr, st, dt, n_steps, gamma, kT, seed, fixed


def _to_dev(pos, vel, force, mass, node_ptr, st, dt, n_steps, gamma, kT, seed, fixed):
    from matdeeplearn_amd import ops
    d = dev()
    t = lambda a: torch.from_numpy(np.array(a)).to(d)
    state = ops.MDState(t(st["steps"]), t(st["status"]), t(st["ekin"]))
    return [t(pos), t(vel), t(force), t(mass), t(node_ptr), state, t(dt), t(n_steps), t(gamma), t(kT), t(seed), t(fixed)]


def _launch(inp, **kw):
    from matdeeplearn_amd import ops
    a = _to_dev(*inp)
    out = ops.md_step(*a, max_disp=MAX_DISP, **kw)
    assert out is a[5]
    return a[0], a[1], a[5]


def _close(got, ref, node_ptr, name):
    """rows node_ptr[b] .. node_ptr[b + 1] of got, for every b: within 1e-12 of the largest magnitude of those rows of the reference —
    the project's bound for fire_step, taken per structure so that one large structure cannot hide the others"""
    got, worst = got.cpu().numpy(), 0.0
    assert got.shape == ref.shape and np.isfinite(ref).all(), name
    for b in range(len(node_ptr) - 1):
        g, r = got[node_ptr[b]:node_ptr[b + 1]], ref[node_ptr[b]:node_ptr[b + 1]]
        if r.size == 0:
            continue
        scale, err = np.abs(r).max(), np.abs(g - r).max()
        worst = max(worst, err / scale if scale > 0 else err)
        assert err <= 1e-12 * scale, (name, b, err, scale)
    print("%s: largest error %.3e of a structure's largest magnitude (bound 1e-12)" % (name, worst))


def test_md_step_matches_the_host_reference_in_every_branch():
    """On the MI355X: pos 8.9e-17, vel 4.4e-16, ekin 2.0e-16 of a structure's largest magnitude at worst."""
    inp = _md_inputs()
    pos, vel, force, mass, node_ptr, st, dt, n_steps, gamma, kT, seed, fixed = inp
    B = len(SIZES)
    rpos, rvel, rst, diag = tmh.md_reference(*inp, max_disp=MAX_DISP)
    # the reference's own values: every branch is there, and no guard decision is marginal
    want = {FIRST: "nve", NVE: "nve", LANGEVIN: "langevin", COLD: "langevin", SOME_FIXED: "langevin", EMPTY: "nve", ALL_FIXED: "nve",
            LATER: "langevin", CLOSING: "closing", FINISHED: "stopped", GUARD_BIG: "refused", GUARD_NAN: "refused", REFUSED_BEFORE: "stopped"}
    assert {b: diag[b]["branch"] for b in range(B)} == want
    assert st["steps"][FIRST] == 0 and st["steps"][NVE] > 0 and st["steps"][GUARD_NAN] == 0 and st["steps"][GUARD_BIG] > 0
    for b in range(B):
        disp = diag[b]["disp"]
        assert (np.isnan(disp) | (np.abs(disp - MAX_DISP) >= 1e-3)).all(), (b, disp)
    assert np.isfinite(diag[GUARD_BIG]["disp"]).all() and (diag[GUARD_BIG]["disp"] > MAX_DISP).sum() == 1
    assert np.isnan(diag[GUARD_NAN]["disp"]).sum() == 1 and (diag[GUARD_NAN]["disp"][np.isfinite(diag[GUARD_NAN]["disp"])] < MAX_DISP).all()

    dpos, dvel, state = _launch(inp)
    for k in ("steps", "status"):
        assert np.array_equal(getattr(state, k).cpu().numpy(), rst[k]), (k, getattr(state, k), rst[k])
    assert state.status.cpu().tolist() == [0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 2, 2, 2]
    _close(dpos, rpos, node_ptr, "pos")
    _close(dvel, rvel, node_ptr, "vel")
    _close(state.ekin, rst["ekin"], np.arange(B + 1), "ekin")
    gpos, gvel = dpos.cpu().numpy(), dvel.cpu().numpy()
    seg = lambda b: slice(node_ptr[b], node_ptr[b + 1])
    # stopped before: every bit is what went in, ekin included
    for b in (FINISHED, REFUSED_BEFORE):
        assert np.array_equal(gpos[seg(b)], pos[seg(b)]) and np.array_equal(gvel[seg(b)], vel[seg(b)]) and float(state.ekin[b]) == -1.0
        assert int(state.steps[b]) == st["steps"][b] and int(state.status[b]) == st["status"][b]
    # closing and refused: the positions keep their bits; a refusal at the first step leaves the velocities alone too
    for b in (CLOSING, GUARD_BIG, GUARD_NAN, ALL_FIXED):
        assert np.array_equal(gpos[seg(b)], pos[seg(b)]), b
    assert np.array_equal(gvel[seg(GUARD_NAN)], vel[seg(GUARD_NAN)]) and int(state.steps[GUARD_BIG]) == st["steps"][GUARD_BIG]
    assert np.isfinite(gpos).all() and np.isfinite(gvel).all()
    # fixed atoms stay where they are and lose their velocity; free atoms of running structures move
    running = np.zeros(len(pos), bool)
    for b in range(B):
        running[seg(b)] = diag[b]["branch"] in ("nve", "langevin")
    fx = (fixed != 0) & running
    assert fx.any() and np.array_equal(gpos[fx], pos[fx]) and not gvel[fx].any()
    assert (gpos[running & (fixed == 0)] != pos[running & (fixed == 0)]).any(1).all()
    assert float(state.ekin[ALL_FIXED]) == 0.0 and float(state.ekin[EMPTY]) == 0.0 and int(state.steps[EMPTY]) == st["steps"][EMPTY] + 1


def test_md_step_repeats_its_bits_alone_and_in_any_batch():
    from matdeeplearn_amd import ops
    inp = _md_inputs()
    pos, vel, force, mass, node_ptr, st, dt, n_steps, gamma, kT, seed, fixed = inp
    dpos, dvel, state = _launch(inp)
    dpos2, dvel2, state2 = _launch(inp)
    assert torch.equal(dpos, dpos2) and torch.equal(dvel, dvel2)
    for k in ("steps", "status", "ekin"):
        assert torch.equal(getattr(state, k), getattr(state2, k)), k
    # each structure alone, with its key
    for b in range(len(SIZES)):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        one = {k: v[b:b + 1] for k, v in st.items()}
        alone = (pos[a:e], vel[a:e], force[a:e], mass[a:e], np.array([0, e - a]), one, dt[b:b + 1], n_steps[b:b + 1], gamma[b:b + 1],
                 kT[b:b + 1], seed[b:b + 1], fixed[a:e])
        apos, avel, astate = _launch(alone)
        assert torch.equal(apos, dpos[a:e]) and torch.equal(avel, dvel[a:e]), b
        for k in ("steps", "status", "ekin") if e > a else ():      # (N == 0 is no launch by the C ABI: nothing counts the empty batch's steps)
            assert torch.equal(getattr(astate, k), getattr(state, k)[b:b + 1]), (b, k)
    # a plain integer seed s is the key s + b
    arg = list(inp)
    arg[10] = 1000 + np.arange(len(SIZES))
    by_tensor = _launch(arg)
    a = _to_dev(*inp)
    ops.md_step(*a[:10], 1000, a[11], MAX_DISP)
    assert torch.equal(a[0], by_tensor[0]) and torch.equal(a[1], by_tensor[1]) and not torch.equal(a[0], dpos)
    # without a thermostat no random number enters: two seeds, the same bits
    arg[8] = np.zeros(len(SIZES))
    nve1 = _launch(arg)
    arg[10] = 77 + np.arange(len(SIZES))
    nve2 = _launch(arg)
    assert torch.equal(nve1[0], nve2[0]) and torch.equal(nve1[1], nve2[1]) and torch.equal(nve1[2].ekin, nve2[2].ekin)
    assert not torch.equal(nve1[0], dpos)


def test_md_step_rejects_bad_arguments():
    from matdeeplearn_amd import ops
    names = ("pos", "vel", "force", "mass", "node_ptr", "state", "dt", "n_steps", "gamma", "kT", "seed", "fixed")
    args = dict(zip(names, _to_dev(*_md_inputs())))

    def bad(**kw):
        a = dict(args, **kw)
        with pytest.raises(ops.MdlError):
            ops.md_step(*[a[k] for k in names], a.get("max_disp", MAX_DISP))

    bad(pos=args["pos"].float())
    bad(vel=args["vel"][:-1])
    bad(pos=args["pos"].t().contiguous().t())                               # not contiguous: the update is in place
    bad(force=args["force"].double())
    bad(mass=args["mass"].float())
    bad(mass=args["mass"][:-1])
    bad(mass=torch.where(torch.arange(args["mass"].numel(), device=dev()) == 3, 0.0, args["mass"]))
    bad(node_ptr=args["node_ptr"].to(torch.int32))
    bad(dt=args["dt"].float())
    bad(dt=args["dt"][:-1])
    bad(dt=-args["dt"])
    bad(gamma=args["gamma"] - 1.0)
    bad(kT=args["kT"] - 1.0)
    bad(n_steps=args["n_steps"].long())
    bad(seed=args["seed"].to(torch.int32))
    bad(fixed=args["fixed"].to(torch.int32))
    bad(state=None)
    bad(state=ops.md_state(len(SIZES) - 1, dev()))
    bad(pos=args["pos"].cpu())
    bad(max_disp=0.0)
    bad(max_disp=float("nan"))
    # nothing above moved anything
    ref = _to_dev(*_md_inputs())
    assert torch.equal(args["pos"], ref[0]) and torch.equal(args["vel"], ref[1]) and torch.equal(args["state"].steps, ref[5].steps)
    z = lambda *s, dtype=torch.float64: torch.zeros(*s, dtype=dtype, device=dev())
    ops.md_step(z(0, 3), z(0, 3), z(0, 3, dtype=torch.float32), z(0), z(1, dtype=torch.int64), ops.md_state(0, dev()), 0.1, 5)     # B = 0: no launch
    assert tuple(ops.md_velocities(z(0), z(1, dtype=torch.int64), 1.0).shape) == (0, 3)


def test_md_velocities_match_the_host_reference():
    """On the MI355X: 6.1e-16 of a structure's largest magnitude at worst, the noise alone 4.4e-16."""
    from matdeeplearn_amd import ops
    pos, vel, force, mass, node_ptr, st, dt, n_steps, gamma, kT, seed, fixed = _md_inputs()
    d = dev()
    t = lambda a: torch.from_numpy(np.array(a)).to(d)
    seg = lambda b: slice(node_ptr[b], node_ptr[b + 1])
    for fx, zero in ((fixed, True), (None, True), (fixed, False)):
        got = ops.md_velocities(t(mass), t(node_ptr), t(kT), t(seed), None if fx is None else t(fx), zero_momentum=zero)
        ref = tmh.md_velocities_reference(mass, node_ptr, kT, seed, fx, zero)
        assert got.dtype == torch.float64 and tuple(got.shape) == (len(mass), 3)
        _close(got, ref, node_ptr, "velocities (fixed %s, zero_momentum %s)" % (fx is not None, zero))
        g = got.cpu().numpy()
        if fx is not None:
            assert not g[fx != 0].any() and (g[(fx == 0) & (np.repeat(kT, SIZES) > 0)] != 0).any(1).all()
        for b in range(len(SIZES)):
            free = np.ones(SIZES[b], bool) if fx is None else fx[seg(b)] == 0
            mv = mass[seg(b)][free, None] * g[seg(b)][free]
            if zero and free.sum() >= 2:
                assert (np.abs(mv.sum(0)) <= 1e-12 * np.abs(mv).sum()).all(), (b, mv.sum(0), np.abs(mv).sum())
            elif free.sum() >= 1 and kT[b] > 0:
                assert np.abs(mv.sum(0)).max() > 1e-6 * np.abs(mv).sum()           # a single atom, or no removal: the momentum stays
    assert torch.equal(got, ops.md_velocities(t(mass), t(node_ptr), t(kT), t(seed), t(fixed), zero_momentum=False))
    # kT = 1, m = 1, nothing removed: the noise itself
    n = 700
    xi = ops.md_velocities(torch.ones(n, dtype=torch.float64, device=d), t(np.array([0, n])), 1.0, seed=12345, zero_momentum=False)
    _close(xi, tmh.md_noise_reference(n, 0, 1, 12345), np.array([0, n]), "noise")
    # one structure's draw does not depend on the batch
    alone = ops.md_velocities(t(mass[seg(7)]), t(np.array([0, SIZES[7]])), t(kT[7:8]), t(seed[7:8]), t(fixed[seg(7)]), zero_momentum=False)
    assert torch.equal(alone, got[seg(7)])


def test_langevin_samples_harmonic_wells_on_the_device():
    """tests/test_md_host.py's Langevin test through ops.md_step, the forces formed on the device: 64 structures of 256 atoms.
    On the MI355X: <k x^2> / kT - 1 = 2.3e-3 (bound 5.5e-2)."""
    from matdeeplearn_amd import ops
    node_ptr, dt, gamma, mass, k, x0 = tmh.langevin_case()
    d, L = dev(), tmh.LANGEVIN
    t = lambda a: torch.from_numpy(np.array(a)).to(d)
    dk, dx0, dmass, dptr, ddt, dgamma = t(k), t(x0), t(mass), t(node_ptr), t(dt), t(gamma)
    pos, vel, state = dx0.clone(), torch.zeros_like(dx0), ops.md_state(len(dt), d)
    n_steps = torch.full((len(dt),), L["steps"], dtype=torch.int32, device=d)
    for _ in range(L["steps"] + 1):
        ops.md_step(pos, vel, (-dk * (pos - dx0)).float(), dmass, dptr, state, ddt, n_steps, dgamma, L["kT"], L["seed"], max_disp=1e9)
    assert (state.status == 1).all() and (state.steps == L["steps"]).all()
    tmh.langevin_check(pos.cpu().numpy(), k, x0)


# ---------------------------------------------------------------------------------------------
# forces.md
# ---------------------------------------------------------------------------------------------
def _oracle_model():
    from matdeeplearn_amd import models
    model = models.CGCNN(DS(), dim1=64, dim2=64, gc_count=2, post_fc_count=1)
    model.load_state_dict(trh.cgcnn_case().state_dict)
    return model.to(dev()).eval()


def test_md_nve_follows_the_fp64_reference_trajectory_at_held_lists():
    """On the MI355X: the atoms travel up to 1.03 A and end 1.2e-7 A from the fp64 trajectory (MD_TRAJ_BOUND 3.2e-4 A); prediction + ekin
    leaves its first value by 3.8e-7, 1.7e-6, 6.1e-7, 4.2e-7, 3.3e-6, 5.9e-6 per structure, the fp64 trajectory by 3.8e-7, 1.7e-6, 5.1e-7,
    3.8e-7, 3.3e-6, 5.9e-6 (the bound: twice that plus one fp32 spacing of the prediction, 4.7e-10 ... 1.9e-9)."""
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    ref_pos, ref_vel, ref_epot, ref_ekin, _ = tmh.cgcnn_md_reference()
    model, B, steps = _oracle_model(), len(case.structs), tmh.MD_ARGS["steps"]
    with ops.deterministic():
        res = forces.md(model, case.structs, DIST_RANGE, tmh.md_masses(case), velocities=tmh.md_initial_velocities(case), rebuild_every=0,
                        **tmh.MD_ARGS)
        ff = forces.ForceField(model, case.structs, DIST_RANGE)             # the lists of the initial positions
        ff.set_positions(res.positions)
        e_held, f_held = ff.evaluate()
    assert res.positions.dtype == torch.float64 and res.velocities.dtype == torch.float64 and res.ekin.dtype == torch.float64
    assert res.steps.dtype == torch.int32 and res.status.dtype == torch.int32 and res.forces.dtype == torch.float32
    assert (res.steps == steps).all() and (res.status == 1).all()
    assert tuple(res.epot_trace.shape) == (steps + 1, B) and tuple(res.ekin_trace.shape) == (steps + 1, B)
    assert torch.equal(res.energy, e_held) and torch.equal(res.forces, f_held) and torch.equal(res.epot_trace[-1], res.energy)
    assert torch.equal(res.ekin_trace[-1], res.ekin)
    dev_ = np.sqrt(((res.positions.cpu().numpy() - ref_pos) ** 2).sum(1)).max()
    travelled = np.sqrt(((res.positions.cpu().numpy() - case.p["pos"]) ** 2).sum(1)).max()
    total = res.epot_trace.double().cpu().numpy() + res.ekin_trace.cpu().numpy()
    exc = np.abs(total - total[0]).max(0)
    ref_total = ref_epot + ref_ekin
    ref_exc = np.abs(ref_total - ref_total[0]).max(0)
    resolution = np.spacing(np.abs(res.epot_trace.cpu().numpy()).max(0).astype(np.float32)).astype(np.float64)
    print("largest distance from the reference trajectory %.3e A (MD_TRAJ_BOUND %.1e); travelled %.3e A" % (dev_, tmh.MD_TRAJ_BOUND, travelled))
    print("excursion of prediction + ekin", exc, "of the fp64 trajectory", ref_exc, "fp32 resolution of the prediction", resolution)
    print("velocities: largest difference %.3e of %.3e" % (np.abs(res.velocities.cpu().numpy() - ref_vel).max(), np.abs(ref_vel).max()))
    assert travelled >= 0.1
    assert dev_ <= tmh.MD_TRAJ_BOUND
    assert (ref_exc <= tmh.MD_ENERGY_EXCURSION).all()
    assert (exc <= 2.0 * ref_exc + resolution).all()


def test_md_with_a_thermostat_repeats_its_bits_and_rebuilds():
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    model, masses = _oracle_model(), tmh.md_masses(case)
    args = dict(dt=1.0, steps=6, kT=2e-5, gamma=0.05)
    with ops.deterministic():
        res = forces.md(model, case.structs, DIST_RANGE, masses, seed=3, **args)             # rebuild_every = 1, velocities drawn
        again = forces.md(model, case.structs, DIST_RANGE, masses, seed=3, **args)
        other = forces.md(model, case.structs, DIST_RANGE, masses, seed=4, **args)
    for a, b in zip(res, again):
        assert torch.equal(a, b)
    assert not torch.equal(res.positions, other.positions) and not torch.equal(res.velocities, other.velocities)
    assert ((res.status == 0) | (res.status == 1)).all() and (res.status == 1).all() and (res.steps == 6).all()
    assert not torch.isnan(res.epot_trace).any() and not torch.isnan(res.ekin_trace).any() and (res.ekin > 0).all()
    pos = res.positions.cpu().numpy()
    assert (pos != case.p["pos"]).any(1).all()
    # the returned energy belongs to the returned positions on REBUILT lists: the existing path gives it back
    node_ptr = case.p["node_ptr"]
    with ops.deterministic():
        final = [dict(s, positions=pos[a:b]) for s, a, b in zip(case.structs, node_ptr[:-1], node_ptr[1:])]
        e1, f1, _ = forces.energy_and_forces(model, final, DIST_RANGE)
    assert torch.equal(res.energy, e1) and torch.equal(res.forces, f1)
    # fixed atoms, one temperature per structure, and the guard: a max_disp below the first step stops every structure where it is
    fixed = np.zeros(len(pos), bool)
    fixed[::3] = True
    held = forces.md(model, case.structs, DIST_RANGE, masses, 1.0, 3, kT=np.linspace(1e-5, 3e-5, len(case.structs)), gamma=0.05, fixed=fixed)
    assert np.array_equal(held.positions.cpu().numpy()[fixed], case.p["pos"][fixed]) and not held.velocities.cpu().numpy()[fixed].any()
    stopped = forces.md(model, case.structs, DIST_RANGE, masses, 1.0, 3, kT=2e-5, gamma=0.05, max_disp=1e-9, check_every=1)
    assert (stopped.status == 2).all() and (stopped.steps == 0).all() and np.array_equal(stopped.positions.cpu().numpy(), case.p["pos"])
    assert torch.isnan(stopped.epot_trace[1:]).all() and not torch.isnan(stopped.epot_trace[0]).any()


def test_md_refuses_training_mode_and_bad_arguments():
    from matdeeplearn_amd import forces, ops
    structs = tgf._bulk_structures(2, seed=4, lo=4, hi=8)
    n = sum(len(s["positions"]) for s in structs)
    model = _oracle_model()
    with pytest.raises(ops.MdlError, match="masses must be"):
        forces.md(model, structs, DIST_RANGE, np.ones(n + 1), 1.0, 1)
    with pytest.raises(ops.MdlError, match="mass must be > 0"):
        forces.md(model, structs, DIST_RANGE, np.zeros(n), 1.0, 1, velocities=np.zeros((n, 3)))
    with pytest.raises(ops.MdlError, match="dt must be > 0"):
        forces.md(model, structs, DIST_RANGE, np.ones(n), 0.0, 1)
    with pytest.raises(ops.MdlError, match="steps"):
        forces.md(model, structs, DIST_RANGE, np.ones(n), 1.0, -1)
    model.train()
    with pytest.raises(ops.MdlError, match="eval"):
        forces.md(model, structs, DIST_RANGE, np.ones(n), 1.0, 1)
