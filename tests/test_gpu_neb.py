"""GPU checks of the nudged elastic band: ops.neb_step (the band mode of mdl_fire_step: the band-force kernel of csrc/neb.hip, then
the FIRE kernel over whole bands) against the fp64 restatements that tests/test_neb_host.py and tests/test_relax_host.py own, its
repeatability, and forces.neb against the fp64 reference trajectory of the oracle CGCNN at held neighbour lists (bound:
NEB_TRAJ_BOUND of the host file, the reference's own sensitivity to force errors of the size the force tests allow)."""
import numpy as np
import pytest
import torch

import test_neb_host as tnh
from test_gpu_forces import DIST_RANGE, DS, dev

pytestmark = pytest.mark.gpu


def _to_dev(c):
    """the host batch `c` (test_neb_host.neb_batch / sub_batch) as the operands of ops.neb_step"""
    from matdeeplearn_amd import ops
    d = dev()
    t = lambda a: torch.from_numpy(np.array(a)).to(d)
    state = ops.neb_state(t(c.image_ptr), t(c.band_ptr), t(c.fixed))
    for k in ops.FireState.__slots__:
        setattr(state, k, t(c.state[k]))
    return dict(pos=t(c.pos), vel=t(c.vel), force=t(c.force), energy=t(c.energy), cell=t(c.cell), pbc=t(c.pbc), state=state, fmax=t(c.fmax),
                spring=t(c.spring), climb=t(c.climb))


def _step(c, **kw):
    from matdeeplearn_amd import ops
    a = _to_dev(c)
    a.update(kw)
    out = ops.neb_step(a["pos"], a["vel"], a["force"], a["energy"], a["cell"], a["pbc"], a["state"], a["fmax"], a["spring"], a["climb"])
    assert out is a["state"]
    return a


def _band_scale(x, ptr):
    """the largest magnitude of x per band (rows ptr[b] .. ptr[b + 1]), repeated over the band's rows; 1 where a band is all zero"""
    out = np.ones(len(x))
    for a, e in zip(ptr[:-1], ptr[1:]):
        if e > a and np.abs(x[a:e]).max() > 0:
            out[a:e] = np.abs(x[a:e]).max()
    return out


def test_neb_step_matches_the_host_reference_in_every_role():
    from matdeeplearn_amd import ops
    c = tnh.neb_batch()
    node_ptr = c.image_ptr[c.band_ptr]
    a = _step(c)
    state = a["state"]
    assert np.array_equal(state.band_node_ptr.cpu().numpy(), node_ptr)
    mask = state.fixed.cpu().numpy().astype(bool)
    rbf, rtf, rseg, rclimber, _ = tnh.neb_reference(c.pos, c.force, c.energy, c.image_ptr, c.band_ptr, c.cell, c.pbc, c.spring, c.climb, mask)
    # the band force: fp64, rounded once — within one fp32 spacing of the image's largest component
    bf = state.band_force.cpu().numpy()
    worst = 0.0
    for s in range(c.I):
        rows = slice(c.image_ptr[s], c.image_ptr[s + 1])
        big = np.abs(rbf[rows]).max()
        err = np.abs(bf[rows].astype(np.float64) - rbf[rows]).max()
        worst = max(worst, err / np.spacing(np.float32(big)) if big > 0 else err)
        assert err <= np.spacing(np.float32(big)) if big > 0 else not bf[rows].any(), (s, err, big)
    print("band_force: worst error %.3f fp32 spacings of the image's largest component" % worst)
    assert np.array_equal(state.climber.cpu().numpy(), rclimber), (state.climber, rclimber)
    for name, got, ref in (("tangent_force", state.tangent_force, rtf), ("seg_len", state.seg_len, rseg)):
        err = np.abs(got.cpu().numpy() - ref) / _band_scale(ref, c.band_ptr)
        print("%s: max err %.3e of the band's largest (bound 1e-12)" % (name, err.max()))
        assert err.max() <= 1e-12, name
    # the update: neb_reference rounded once to fp32, then fire_reference with every band as one structure (the host file has
    # shown that this batch takes every branch of it, none marginally)
    rpos, rvel, rst = tnh.neb_step_reference(c.pos, c.vel, c.force, c.energy, c.image_ptr, c.band_ptr, c.cell, c.pbc, c.spring, c.climb, c.state,
                                             c.fmax, c.fixed)[:3]
    for k in ("n_pos", "steps", "done"):
        assert np.array_equal(getattr(state, k).cpu().numpy(), rst[k]), (k, getattr(state, k), rst[k])
    assert np.array_equal(state.dt.cpu().numpy(), rst["dt"]) and np.array_equal(state.alpha.cpu().numpy(), rst["alpha"])
    for name, got, ref in (("pos", a["pos"], rpos), ("vel", a["vel"], rvel)):
        err = np.abs(got.cpu().numpy() - ref).max(1) / _band_scale(ref, node_ptr)
        print("%s: max err %.3e of the band's largest (bound 1e-12)" % (name, err.max()))
        assert err.max() <= 1e-12, name
    seen = state.fmax_seen.cpu().numpy()
    assert (np.abs(seen - rst["fmax_seen"]) <= np.spacing(np.abs(rst["fmax_seen"]))).all(), (seen, rst["fmax_seen"])
    # bands the update must not touch: bitwise what went in
    for b in (tnh.TWO, tnh.LATCHED, tnh.CONVERGING):
        sl = slice(node_ptr[b], node_ptr[b + 1])
        assert np.array_equal(a["pos"].cpu().numpy()[sl], c.pos[sl]) and np.array_equal(a["vel"].cpu().numpy()[sl], c.vel[sl]), b
        for k in ("dt", "alpha", "n_pos", "steps"):
            assert getattr(state, k).cpu().numpy()[b] == c.state[k][b], (b, k)
        assert int(state.done[b]) == 1
    # end images and fixed atoms stay; the free atoms of moving bands move
    moving = np.zeros(c.N, bool)
    for b in (tnh.COINCIDE, tnh.TRICLINIC, tnh.TIES, tnh.NOCLIMB):
        moving[node_ptr[b]:node_ptr[b + 1]] = True
    assert np.array_equal(a["pos"].cpu().numpy()[mask], c.pos[mask]) and not a["vel"].cpu().numpy()[mask & moving].any()
    assert (a["pos"].cpu().numpy()[moving & ~mask] != c.pos[moving & ~mask]).any(1).all()
    # climbing switched off everywhere, and scalar operands
    b = _step(c, climb=False, spring=1.0, fmax=0.05)
    off = tnh.neb_reference(c.pos, c.force, c.energy, c.image_ptr, c.band_ptr, c.cell, c.pbc, np.ones(c.B), np.zeros(c.B), mask)
    assert (b["state"].climber == -1).all()
    assert np.abs(b["state"].band_force.cpu().numpy() - off[0]).max() <= np.spacing(np.float32(np.abs(off[0]).max()))
    assert np.abs(b["state"].tangent_force.cpu().numpy() - off[1]).max() <= 1e-12 * np.abs(off[1]).max()
    # the plain call is what it was: fire_step on the device's band force moves the bands to the same bits
    p = _to_dev(c)
    plain = ops.FireState(*[getattr(p["state"], k) for k in ops.FireState.__slots__])
    ops.fire_step(p["pos"], p["vel"], state.band_force, state.band_node_ptr, plain, p["fmax"], state.fixed)
    assert torch.equal(p["pos"], a["pos"]) and torch.equal(p["vel"], a["vel"])
    for k in ops.FireState.__slots__:
        assert torch.equal(getattr(plain, k), getattr(state, k)), k


def test_neb_step_is_repeatable_and_a_band_alone_gets_its_bits():
    from matdeeplearn_amd import ops
    c = tnh.neb_batch()
    a, again = _step(c), _step(c)
    assert torch.equal(a["pos"], again["pos"]) and torch.equal(a["vel"], again["vel"])
    for k in ops.NebState.__slots__:
        assert torch.equal(getattr(a["state"], k), getattr(again["state"], k)), k
    for b in range(c.B):
        one = tnh.sub_batch(c, b)
        o = _step(one)
        assert torch.equal(o["pos"], a["pos"][one.rows]) and torch.equal(o["vel"], a["vel"][one.rows]), b
        assert torch.equal(o["state"].band_force, a["state"].band_force[one.rows]), b
        for k in ("tangent_force", "seg_len"):
            assert torch.equal(getattr(o["state"], k), getattr(a["state"], k)[one.images]), (b, k)
        for k in ops.FireState.__slots__:
            assert torch.equal(getattr(o["state"], k), getattr(a["state"], k)[b:b + 1]), (b, k)
        cl = int(a["state"].climber[b])
        assert int(o["state"].climber[0]) == (cl - one.images.start if cl >= 0 else -1), b


def _oracle_model():
    from matdeeplearn_amd import models
    model = models.CGCNN(DS(), dim1=64, dim2=64, gc_count=2, post_fc_count=1)
    model.load_state_dict(tnh.neb_case().state_dict)
    return model.to(dev()).eval()


def test_neb_follows_the_fp64_reference_trajectory_at_held_lists():
    from matdeeplearn_amd import forces, ops
    case = tnh.neb_case()
    ref_pos, ref_st, ref_climber, _ = tnh.neb_cgcnn_reference()
    model = _oracle_model()
    I, B = len(case.structs), len(case.bands)
    with ops.deterministic():
        res = forces.neb(model, case.bands, DIST_RANGE, rebuild_every=0, **tnh.NEB_ARGS)
        ff = forces.ForceField(model, case.structs, DIST_RANGE)               # the lists of the initial band
        ff.set_positions(res.positions)
        e_held, f_held = ff.evaluate()
    assert res.positions.dtype == torch.float64 and res.forces.dtype == torch.float32 and res.band_forces.dtype == torch.float32
    assert res.converged.dtype == torch.bool and res.steps.dtype == torch.int32 and res.climber.dtype == torch.int32
    dev_ = np.sqrt(((res.positions.cpu().numpy() - ref_pos) ** 2).sum(1)).max()
    print("largest distance from the reference trajectory %.3e A (NEB_TRAJ_BOUND %.1e)" % (dev_, tnh.NEB_TRAJ_BOUND))
    assert dev_ <= tnh.NEB_TRAJ_BOUND
    assert np.array_equal(res.climber.cpu().numpy(), ref_climber) and np.array_equal(res.steps.cpu().numpy(), ref_st["steps"])
    assert not res.converged.any() and tuple(res.energy.shape) == (I,)
    assert torch.equal(res.energy, e_held) and torch.equal(res.forces, f_held)
    assert np.array_equal(res.band_ptr.cpu().numpy(), case.band_ptr) and np.array_equal(res.node_ptr.cpu().numpy(), case.p["node_ptr"])
    # what is derived from the last evaluation: barrier, path, fmax
    e, bf = res.energy.cpu().numpy(), res.band_forces.double().cpu().numpy()
    for b in range(B):
        i0, i1 = case.band_ptr[b], case.band_ptr[b + 1]
        assert float(res.barrier[b]) == np.float32(e[i0 + 1:i1 - 1].max() - e[i0])
        rows = slice(case.p["node_ptr"][i0], case.p["node_ptr"][i1])
        assert abs(float(res.fmax[b]) - np.sqrt((bf[rows] ** 2).sum(1)).max()) <= 1e-6 * float(res.fmax[b])
        path = res.path[i0:i1].cpu().numpy()
        assert path[0] == 0 and (np.diff(path) > 0).all()
    p = res.positions.cpu().numpy()
    nb = tnh.neb_reference(p, res.forces.cpu().numpy(), e, case.p["node_ptr"], case.band_ptr, case.p["cell"], case.p["pbc"],
                           [tnh.NEB_ARGS["spring"]] * B, [1] * B)
    assert np.abs(res.tangent_force.cpu().numpy() - nb[1]).max() <= 1e-9 * np.abs(nb[1]).max()


def test_neb_with_rebuilt_lists_is_bitwise_repeatable():
    from matdeeplearn_amd import forces, ops
    case = tnh.neb_case()
    model = _oracle_model()
    args = dict(tnh.NEB_ARGS, steps=6, climb_after=3)
    with ops.deterministic():
        res = forces.neb(model, case.bands, DIST_RANGE, rebuild_every=1, **args)
        again = forces.neb(model, case.bands, DIST_RANGE, rebuild_every=1, **args)
    for x, y in zip(res, again):
        assert torch.equal(x, y)
    assert (res.steps == 6).all() and (res.climber >= 0).all()
    moved = (res.positions.cpu().numpy() != case.p["pos"]).any(1)
    ends = np.zeros(len(moved), bool)
    for b in range(len(case.bands)):
        for s in (case.band_ptr[b], case.band_ptr[b + 1] - 1):
            ends[case.p["node_ptr"][s]:case.p["node_ptr"][s + 1]] = True
    assert not moved[ends].any() and moved[~ends].all()
    # climbing held back: below climb_after no image climbs
    with ops.deterministic():
        early = forces.neb(model, case.bands, DIST_RANGE, rebuild_every=1, **dict(args, steps=2))
    assert (early.climber == -1).all() and (early.steps == 2).all()


def test_neb_refuses_bad_arguments():
    from matdeeplearn_amd import forces, ops
    case = tnh.neb_case()
    model = _oracle_model()
    model.train()
    with pytest.raises(ops.MdlError, match="eval"):
        forces.neb(model, case.bands, DIST_RANGE, steps=1)
    model.eval()
    short = dict(case.bands[0][1], positions=case.bands[0][1]["positions"][:-1], numbers=case.bands[0][1]["numbers"][:-1])
    with pytest.raises(ops.MdlError, match="unequal atom counts"):
        forces.neb(model, [[case.bands[0][0], short, case.bands[0][2]]], DIST_RANGE, steps=1)
    with pytest.raises(ops.MdlError, match="non-empty"):
        forces.neb(model, [], DIST_RANGE, steps=1)
    d = dev()
    with pytest.raises(ops.MdlError, match="unequal atom counts"):
        ops.neb_state(torch.tensor([0, 2, 4, 5], device=d), torch.tensor([0, 3], device=d))
    with pytest.raises(ops.MdlError, match="span"):
        ops.neb_state(torch.tensor([0, 2, 4, 6], device=d), torch.tensor([0, 2], device=d))
    with pytest.raises(ops.MdlError, match="non-decreasing"):
        ops.neb_state(torch.tensor([0, 2, 1, 6], device=d), torch.tensor([0, 3], device=d))
    with pytest.raises(ops.MdlError, match="int64"):
        ops.neb_state(torch.tensor([0, 2, 4, 6], device=d, dtype=torch.int32), torch.tensor([0, 3], device=d))
    c = tnh.sub_batch(tnh.neb_batch(), tnh.TRICLINIC)
    good = _to_dev(c)

    def bad(match="neb_step:", **kw):
        a = dict(good)
        a.update(kw)
        with pytest.raises(ops.MdlError, match=match):
            ops.neb_step(a["pos"], a["vel"], a["force"], a["energy"], a["cell"], a["pbc"], a["state"], a["fmax"], a["spring"], a["climb"],
                         **a.get("const", {}))

    bad(pos=good["pos"].float())                                             # dtypes
    bad(force=good["force"].double())
    bad(energy=good["energy"].double())
    bad(cell=good["cell"].float())
    bad(pbc=good["pbc"].long())
    bad(fmax=good["fmax"].float())
    bad(spring=good["spring"].float())
    bad(vel=good["vel"][:-1])                                                # shapes
    bad(pos=good["pos"].t().contiguous().t())
    bad(energy=good["energy"][:-1])
    bad(cell=good["cell"][:-1])
    bad(pbc=good["pbc"][:-1])
    bad(spring=good["spring"].repeat(2))
    bad(climb=good["climb"].repeat(2))
    bad(state=ops.fire_state(1, device=d))
    wrong = good["state"].clone()
    wrong.seg_len = wrong.seg_len[:-1]
    bad(state=wrong)
    wrong = good["state"].clone()
    wrong.climber = wrong.climber.long()
    bad(state=wrong)
    bad(match="HIP device", energy=good["energy"].cpu())                     # devices
    bad(match="HIP device", pos=good["pos"].cpu())
    bad(const={"max_step": 0.1})
    bad(match="mdl_fire_step", const={"maxstep": 0.0})                       # refused by the library
    ref = _to_dev(c)                                                         # nothing above moved anything
    assert torch.equal(good["pos"], ref["pos"]) and torch.equal(good["vel"], ref["vel"]) and torch.equal(good["state"].steps, ref["state"].steps)
