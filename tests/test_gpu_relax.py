"""GPU checks of the relaxation path: the batched FIRE update of csrc/relax.hip (ops.fire_step) against the fp64 restatement that
tests/test_relax_host.py owns, forces.ForceField against the existing entry points (bit for bit), and forces.relax against the
fp64 reference trajectory of the oracle CGCNN at held neighbour lists (bound: TRAJ_BOUND of the host file, the reference's own
sensitivity to force errors of the size the force tests allow)."""
import numpy as np
import pytest
import torch

import test_gpu_forces as tgf
import test_relax_host as trh
from test_gpu_forces import DIST_RANGE, DS, dev

pytestmark = pytest.mark.gpu

SIZES = [1, 2, 7, 64, 65, 0, 300, 513, 33]      # one atom, a pair, < one wave, exactly one wave, a wave + 1, empty, 2 and 3 passes of 256
FIRST, FREE, RESET, CLAMP, LATCHED, EMPTY, CONVERGING, ACCEL, ALL_FIXED = range(9)


def _fire_inputs():
    """seeded inputs that put every branch of the update into one launch (the roles above, by structure)"""
    rng = np.random.default_rng(11)
    node_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    N, B = int(node_ptr[-1]), len(SIZES)
    seg = lambda b: slice(node_ptr[b], node_ptr[b + 1])
    force = rng.normal(size=(N, 3)).astype(np.float32)
    force[seg(FIRST)] *= 0.5
    force[seg(FREE)] *= 0.3
    force[seg(ACCEL)] *= 0.02
    sign = np.ones(N)
    sign[seg(RESET)] = -1.0                                         # P < 0 there, P > 0 elsewhere
    vel = sign[:, None] * (force.astype(np.float64) + 0.05 * rng.normal(size=(N, 3))) * 0.7
    pos = rng.uniform(0.0, 10.0, (N, 3))
    fixed = np.zeros(N, np.uint8)
    fixed[seg(ALL_FIXED)] = 1
    fixed[seg(CLAMP)][::5] = 1
    fixed[seg(ACCEL)][3::7] = 1
    st = trh.new_state(B)
    st["dt"] = np.array([0.1, 0.1, 0.4, 0.95, 0.3, 0.1, 0.2, 0.05, 0.1])
    st["alpha"] = np.array([0.1, 0.1, 0.07, 0.09, 0.05, 0.1, 0.1, 0.08, 0.1])
    st["n_pos"] = np.array([0, 2, 9, 7, 4, 0, 3, 6, 1], np.int32)
    st["steps"] = np.array([0, 3, 12, 9, 30, 0, 4, 8, 2], np.int32)
    st["done"][LATCHED] = 1
    st["fmax_seen"][:] = -1.0
    fmax = np.full(B, 0.05)
    fmax[CONVERGING] = 100.0
    return pos, vel, force, node_ptr, st, fmax, fixed


def _to_dev(pos, vel, force, node_ptr, st, fmax, fixed):
    from matdeeplearn_amd import ops
    d = dev()
    t = lambda a: torch.from_numpy(np.array(a)).to(d)
    state = ops.FireState(*[t(st[k]) for k in ops.FireState.__slots__])
    return t(pos), t(vel), t(force), t(node_ptr), state, t(fmax), t(fixed)


def test_fire_step_matches_the_host_reference_in_every_branch():
    from matdeeplearn_amd import ops
    pos, vel, force, node_ptr, st, fmax, fixed = _fire_inputs()
    B = len(SIZES)
    rpos, rvel, rst, diag = trh.fire_reference(pos, vel, force, node_ptr, st, fmax, fixed)
    # the reference's own values: every branch is there, and no decision is marginal
    want = {FIRST: "first", FREE: "uphill-free", RESET: "reset", CLAMP: "accelerate", LATCHED: "converged", EMPTY: "converged",
            CONVERGING: "converged", ACCEL: "accelerate", ALL_FIXED: "converged"}
    assert {b: diag[b]["branch"] for b in range(B)} == want
    c = trh.FIRE_CONSTANTS
    assert st["dt"][CLAMP] * c["f_inc"] > c["dt_max"] and rst["dt"][CLAMP] == c["dt_max"]
    assert st["dt"][ACCEL] * c["f_inc"] < c["dt_max"] and rst["dt"][ACCEL] == st["dt"][ACCEL] * c["f_inc"]
    assert st["n_pos"][FREE] <= c["n_min"] and rst["dt"][FREE] == st["dt"][FREE]
    assert diag[CONVERGING]["fm"] > 0 and diag[ALL_FIXED]["fm"] == 0 and diag[EMPTY]["fm"] == 0
    moving = [b for b in range(B) if diag[b]["branch"] != "converged"]
    clipped = [b for b in moving if diag[b]["s"] > c["maxstep"]]
    assert clipped and len(clipped) < len(moving), (clipped, moving)          # the clip active and inactive
    for b in range(B):
        if diag[b]["branch"] not in ("converged", "first"):
            assert abs(diag[b]["P"]) >= 1e-3 * diag[b]["abs_fv"], (b, diag[b])
        if b in moving:
            assert abs(diag[b]["s"] - c["maxstep"]) >= 1e-3 * c["maxstep"], (b, diag[b])
        if not st["done"][b] and diag[b]["fm"] > 0:
            assert abs(diag[b]["fm"] - fmax[b]) >= 1e-3 * fmax[b], (b, diag[b])

    def launch():
        dpos, dvel, dforce, dptr, state, dfmax, dfixed = _to_dev(pos, vel, force, node_ptr, st, fmax, fixed)
        out = ops.fire_step(dpos, dvel, dforce, dptr, state, dfmax, dfixed)
        assert out is state
        return dpos, dvel, state

    dpos, dvel, state = launch()
    for k in ("n_pos", "steps", "done"):
        assert np.array_equal(getattr(state, k).cpu().numpy(), rst[k]), (k, getattr(state, k), rst[k])
    for name, got, ref in (("pos", dpos, rpos), ("vel", dvel, rvel), ("dt", state.dt, rst["dt"]), ("alpha", state.alpha, rst["alpha"])):
        err = np.abs(got.cpu().numpy() - ref).max()
        print("%s: max abs err %.3e, scale %.3e (bound 1e-12 of scale)" % (name, err, np.abs(ref).max()))
        assert err <= 1e-12 * np.abs(ref).max(), name
    seen = state.fmax_seen.cpu().numpy()
    assert (np.abs(seen - rst["fmax_seen"]) <= np.spacing(np.abs(rst["fmax_seen"]))).all(), (seen, rst["fmax_seen"])
    # converged structures: what the update must not touch is bitwise what went in
    for b in (LATCHED, EMPTY, CONVERGING, ALL_FIXED):
        sl = slice(node_ptr[b], node_ptr[b + 1])
        assert np.array_equal(dpos.cpu().numpy()[sl], pos[sl]) and np.array_equal(dvel.cpu().numpy()[sl], vel[sl]), b
        for k in ("dt", "alpha", "n_pos", "steps"):
            assert getattr(state, k).cpu().numpy()[b] == st[k][b], (b, k)
        assert int(state.done[b]) == 1
    # fixed atoms of moving structures stay where they are and lose their velocity
    mv = np.zeros(len(pos), bool)
    for b in moving:
        mv[node_ptr[b]:node_ptr[b + 1]] = True
    fx = (fixed != 0) & mv
    assert fx.any() and np.array_equal(dpos.cpu().numpy()[fx], pos[fx]) and not dvel.cpu().numpy()[fx].any()
    assert (dpos.cpu().numpy()[mv & (fixed == 0)] != pos[mv & (fixed == 0)]).any(1).all()
    # no atomics: a second launch from the same inputs gives the same bits
    dpos2, dvel2, state2 = launch()
    assert torch.equal(dpos, dpos2) and torch.equal(dvel, dvel2)
    for k in ops.FireState.__slots__:
        assert torch.equal(getattr(state, k), getattr(state2, k)), k
    # without a mask, with a scalar fmax and constants of the caller's
    free_args = (pos, vel, force, node_ptr, st, 0.05, None)
    dpos3, dvel3, dforce3, dptr3, state3, _, _ = _to_dev(*free_args[:5], fmax, fixed)
    ops.fire_step(dpos3, dvel3, dforce3, dptr3, state3, 0.05, maxstep=0.05, f_dec=0.25)
    rpos3, rvel3, rst3, _ = trh.fire_reference(pos, vel, force, node_ptr, st, 0.05, None, maxstep=0.05, f_dec=0.25)
    assert np.abs(dpos3.cpu().numpy() - rpos3).max() <= 1e-12 * np.abs(rpos3).max()
    assert np.abs(state3.dt.cpu().numpy() - rst3["dt"]).max() <= 1e-12 and np.array_equal(state3.done.cpu().numpy(), rst3["done"])


def test_fire_step_rejects_bad_arguments():
    from matdeeplearn_amd import ops
    args = _to_dev(*_fire_inputs())
    dpos, dvel, dforce, dptr, state, dfmax, dfixed = args
    B = len(SIZES)

    def bad(**kw):
        a = dict(pos=dpos, vel=dvel, force=dforce, node_ptr=dptr, state=state, fmax=dfmax, fixed=dfixed)
        a.update(kw)
        with pytest.raises(ops.MdlError):
            ops.fire_step(a["pos"], a["vel"], a["force"], a["node_ptr"], a["state"], a["fmax"], a["fixed"], **a.get("const", {}))

    bad(pos=dpos.float())
    bad(vel=dvel[:-1])
    bad(pos=dpos.t().contiguous().t())                                     # not contiguous: the update is in place
    bad(force=dforce.double())
    bad(force=dforce[:-1])
    bad(node_ptr=dptr.to(torch.int32))
    bad(fmax=dfmax.float())
    bad(fmax=dfmax[:-1])
    bad(fixed=dfixed.to(torch.int32))
    bad(fixed=dfixed[:-1])
    bad(state=None)
    wrong = state.clone()
    wrong.steps = wrong.steps.long()
    bad(state=wrong)
    short = ops.fire_state(B - 1, device=dev())
    bad(state=short)
    bad(pos=dpos.cpu())
    bad(const={"max_step": 0.1})                                           # an unknown constant
    bad(const={"maxstep": 0.0})                                            # refused by the library
    bad(const={"dt_max": float("nan")})
    # nothing above moved anything
    ref = _to_dev(*_fire_inputs())
    assert torch.equal(dpos, ref[0]) and torch.equal(dvel, ref[1]) and torch.equal(state.steps, ref[4].steps)
    s0 = ops.fire_state(0, device=dev())
    ops.fire_step(torch.zeros(0, 3, dtype=torch.float64, device=dev()), torch.zeros(0, 3, dtype=torch.float64, device=dev()),
                  torch.zeros(0, 3, device=dev()), torch.zeros(1, dtype=torch.int64, device=dev()), s0, 0.05)       # B = 0, N = 0: no launch


# ---------------------------------------------------------------------------------------------
# 2. ForceField is the existing path
# ---------------------------------------------------------------------------------------------
def _model(kind, seed=0):
    from matdeeplearn_amd import models
    torch.manual_seed(seed)
    if kind == "cgcnn":
        m = models.CGCNN(DS(), dim1=64, dim2=64, gc_count=2, post_fc_count=1)
    else:
        m = models.SchNet(DS(), dim1=64, dim2=64, dim3=64, gc_count=2, post_fc_count=1)
    with torch.no_grad():                                        # running statistics that are not the initial ones
        for mod in m.modules():
            if getattr(mod, "running_var", None) is not None:
                mod.running_mean.uniform_(-0.2, 0.2)
                mod.running_var.uniform_(0.5, 1.5)
    return m.to(dev()).eval()


def _same(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and torch.equal(torch.nan_to_num(a, nan=12345.0), torch.nan_to_num(b, nan=12345.0)) \
        and torch.equal(torch.isnan(a), torch.isnan(b))


@pytest.mark.parametrize("kind", ["cgcnn", "schnet"])
def test_force_field_returns_the_bits_of_the_existing_entry_points(kind):
    from matdeeplearn_amd import forces, ops
    model = _model(kind)
    structs = tgf._bulk_structures(8, seed=2, lo=4, hi=30)
    rng = np.random.default_rng(5)
    moved = [dict(s, positions=s["positions"] + 0.05 * _unit(rng, len(s["positions"]))) for s in structs]
    with ops.deterministic():
        pred0, f0, node_ptr = forces.energy_and_forces(model, structs, DIST_RANGE)
        _, _, stress0, _ = forces.energy_forces_stress(model, structs, DIST_RANGE)
        ff = forces.ForceField(model, structs, DIST_RANGE)
        assert ff.positions.dtype == torch.float64 and torch.equal(ff.node_ptr, node_ptr)
        pred, f = ff.evaluate()
        assert _same(pred, pred0) and _same(f, f0)
        pred_s, f_s, stress = ff.evaluate(stress=True)
        assert _same(pred_s, pred0) and _same(f_s, f0) and _same(stress, stress0)
        src0, tgt0 = [t.clone() for t in ff.edges]
        assert src0.dtype == torch.int32 and src0.shape == tgt0.shape
        # moved positions on the HELD lists
        ff.set_positions(np.concatenate([s["positions"] for s in moved]))
        assert torch.equal(ff.edges[0], src0) and torch.equal(ff.edges[1], tgt0)
        pred_h, f_h = ff.evaluate()
        assert not torch.equal(f_h, f0) and not torch.equal(pred_h, pred0)
        # after a rebuild: the existing path on the moved structures
        ff.rebuild()
        pred_m, f_m = ff.evaluate()
        pred1, f1, _ = forces.energy_and_forces(model, moved, DIST_RANGE)
        assert _same(pred_m, pred1) and _same(f_m, f1)
        # set_positions takes a device tensor too; back at the start the first bits return
        ff.set_positions(torch.from_numpy(np.concatenate([s["positions"] for s in structs])).to(dev()))
        ff.rebuild()
        assert _same(ff.evaluate()[1], f0)
        # a slab has no stress: its NaN row is the existing one
        slab = tgf._mixed_structures()[:8]
        ref = forces.energy_forces_stress(model, slab, DIST_RANGE)
        got = forces.ForceField(model, slab, DIST_RANGE).evaluate(stress=True)
        assert torch.isnan(ref[2]).any() and not torch.isnan(ref[2]).all()
        assert _same(got[0], ref[0]) and _same(got[1], ref[1]) and _same(got[2], ref[2])
    assert all(q.grad is None for q in model.parameters())
    with pytest.raises(ops.MdlError):
        ff.set_positions(np.zeros((3, 3)))


def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


# ---------------------------------------------------------------------------------------------
# 3. relax against the fp64 reference trajectory
# ---------------------------------------------------------------------------------------------
def test_relax_follows_the_fp64_reference_trajectory_at_held_lists():
    from matdeeplearn_amd import forces, models, ops
    case = trh.cgcnn_case()
    ref_pos, ref_e, _, _ = trh.cgcnn_reference()
    model = models.CGCNN(DS(), dim1=64, dim2=64, gc_count=2, post_fc_count=1)
    model.load_state_dict(case.state_dict)
    model.to(dev()).eval()
    B = len(case.structs)
    with ops.deterministic():
        e0 = forces.energy_and_forces(model, case.structs, DIST_RANGE)[0]
        res = forces.relax(model, case.structs, DIST_RANGE, rebuild_every=0, **trh.RELAX_ARGS)
        again = forces.relax(model, case.structs, DIST_RANGE, rebuild_every=0, **trh.RELAX_ARGS)
        ff = forces.ForceField(model, case.structs, DIST_RANGE)             # the lists of the initial positions
        ff.set_positions(res.positions)
        e_held, f_held = ff.evaluate()
    assert res.positions.dtype == torch.float64 and res.forces.dtype == torch.float32 and res.fmax.dtype == torch.float32
    assert res.converged.dtype == torch.bool and res.steps.dtype == torch.int32
    dev_ = np.sqrt(((res.positions.cpu().numpy() - ref_pos) ** 2).sum(1)).max()
    print("largest distance from the reference trajectory %.3e A (TRAJ_BOUND %.1e)" % (dev_, trh.TRAJ_BOUND))
    print("energies: start", e0.cpu().numpy(), "end", res.energy.cpu().numpy(), "reference end", ref_e[-1])
    assert dev_ <= trh.TRAJ_BOUND
    assert (res.energy < e0).all()
    assert (res.steps == trh.RELAX_ARGS["steps"]).all() and not res.converged.any()
    assert tuple(res.energy.shape) == (B,) and torch.equal(res.energy, e_held) and torch.equal(res.forces, f_held)
    fm = torch.stack([res.forces.double()[a:b].norm(dim=1).max() for a, b in zip(case.p["node_ptr"][:-1], case.p["node_ptr"][1:])])
    assert torch.allclose(res.fmax.double(), fm, rtol=1e-6, atol=0)
    for a, b in zip(res, again):
        assert torch.equal(a, b)


# ---------------------------------------------------------------------------------------------
# 4. freezing, rebuilding, refusing
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cgcnn", "schnet"])
def test_relax_freezes_converged_structures_rebuilds_and_keeps_fixed_atoms(kind):
    """rebuild_every=1, 10 steps at dt = 3 (seeded, untrained models: forces of order 1e-3 per A, as in the host file).  Half of the
    structures get an fmax above their first force and must come back bit for bit; the others move, downhill, on rebuilt lists."""
    from matdeeplearn_amd import forces, ops
    model = _model(kind)
    structs = tgf._bulk_structures(8, seed=4, lo=4, hi=24)
    p = tgf._pack(structs)
    node_ptr, B, N = p["node_ptr"], 8, p["pos"].shape[0]
    fixed = np.zeros(N, bool)
    fixed[::3] = True
    with ops.deterministic():
        e0, f0, _ = forces.energy_and_forces(model, structs, DIST_RANGE)
        f0 = f0.double().cpu().numpy()
        f0[fixed] = 0.0
        fm0 = np.array([np.sqrt((f0[a:b] ** 2).sum(1)).max() for a, b in zip(node_ptr[:-1], node_ptr[1:])])
        assert (fm0 > 0).all()
        fmax = np.where(np.arange(B) < B // 2, 2.0 * fm0, 0.0)
        res = forces.relax(model, structs, DIST_RANGE, fmax=fmax, steps=10, rebuild_every=1, fixed=fixed, dt=3.0, dt_max=30.0)
    pos = res.positions.cpu().numpy()
    half = node_ptr[B // 2]
    assert np.array_equal(pos[:half], p["pos"][:half])                         # frozen from the first step: the input bits
    assert (res.steps[:B // 2] == 0).all() and res.converged[:B // 2].all()
    assert (res.steps[B // 2:] == 10).all() and not res.converged[B // 2:].any()
    assert np.array_equal(pos[fixed], p["pos"][fixed])
    free_late = ~fixed & (np.arange(N) >= half)
    assert (pos[free_late] != p["pos"][free_late]).any(1).all()
    print("energies: start", e0.cpu().numpy(), "end", res.energy.cpu().numpy())
    assert (res.energy[B // 2:] < e0[B // 2:]).all()
    # the returned energy belongs to the returned positions on REBUILT lists: the existing path gives it back
    with ops.deterministic():
        final = [dict(s, positions=pos[a:b]) for s, a, b in zip(structs, node_ptr[:-1], node_ptr[1:])]
        e1, f1, _ = forces.energy_and_forces(model, final, DIST_RANGE)
    assert torch.equal(res.energy, e1) and torch.equal(res.forces, f1)


def test_relax_refuses_training_mode_and_models_without_forces():
    from matdeeplearn_amd import forces, models, ops
    structs = tgf._bulk_structures(2, seed=4, lo=4, hi=8)
    model = _model("cgcnn")
    model.train()
    with pytest.raises(ops.MdlError, match="eval"):
        forces.relax(model, structs, DIST_RANGE, steps=1)
    gcn = models.GCN(DS(), dim1=64, dim2=64, gc_count=1, post_fc_count=1).to(dev()).eval()
    with pytest.raises(ops.MdlError, match="forces are implemented for CGCNN"):
        forces.relax(gcn, structs, DIST_RANGE, steps=1)
    with pytest.raises(ops.MdlError, match="forces are implemented for CGCNN"):
        forces.ForceField(gcn, structs, DIST_RANGE)
