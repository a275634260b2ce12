"""GPU checks of the time-correlation layer: the kernels of csrc/vacf.hip (ops.md_onstep_velocity, ops.vacf_accumulate) against the
fp64 restatements that tests/test_vacf_host.py owns — every branch in one launch, the on-step velocity to the bit, the correlation
sums within 1e-12 of the sum of the magnitudes of their terms, the same bits alone and in a batch —, and forces.sample with a
forces.Correlate end to end on the oracle CGCNN of tests/test_gpu_md.py: the run is md's / md_npt's to the bit, the velocity stored
with the last frame is bit for bit the one the integrator's closing call stored, and the stored velocities replayed through
ops.vacf_accumulate give the accumulators back bit for bit.

Rounding of a correlation sum: an atom's term is three products and two additions, the centre-of-mass velocity adds a relative
error of a few 2^-53 to either factor, and the sum over at most 513 atoms goes through a tree of depth <= 3 + 6 + 3 — at most
(513 + 8) 2^-53 = 6e-14 of the sum of the magnitudes whatever the order; the bound asked is 1e-12."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_launch_sequence as tgl
import test_gpu_md as tgm
import test_gpu_observe as tgo
import test_md_host as tmh
import test_relax_host as trh
import test_vacf_host as tvh
from test_gpu_forces import DIST_RANGE, dev

pytestmark = pytest.mark.gpu

# one atom, a pair, a wave - 1, exactly one wave, a wave + 1, the workgroup, the workgroup + 1, two rounds of it + 1, and the roles
SIZES = [1, 2, 63, 64, 65, 256, 257, 513, 0, 7, 9, 11]
ONE, PAIR, WAVE_LESS, WAVE, WAVE_MORE, GROUP, GROUP_MORE, BIG, EMPTY, ALL_FIXED, STOPPED, SOME_FIXED = range(12)
N_LAGS = 5
LAGS = ([-1, 0, N_LAGS - 1, N_LAGS + 2], [2, 0, -1, 1])         # two launches: an empty slot, lag 0, the last lag, one past the last


@functools.lru_cache(maxsize=None)
def _inputs():
    rng = np.random.default_rng(41)
    node_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    N, B = int(node_ptr[-1]), len(SIZES)
    vel, force = rng.normal(size=(N, 3)), (rng.normal(size=(N, 3)) * 3.0).astype(np.float32)
    mass, dt = rng.uniform(1.0, 20.0, N), rng.uniform(0.05, 2.0, B)
    fixed = np.zeros(N, np.uint8)
    fixed[node_ptr[ALL_FIXED]:node_ptr[ALL_FIXED + 1]] = 1
    fixed[node_ptr[SOME_FIXED]:node_ptr[SOME_FIXED + 1]][::3] = 1
    fixed[node_ptr[BIG]:node_ptr[BIG + 1]][5::9] = 1
    steps = np.array([0, 3, 0, 1, 7, 0, 2, 5, 4, 1, 6, 0], np.int32)             # no step made yet and steps made, mixed
    status = np.zeros(B, np.int32)
    status[STOPPED] = 2
    return node_ptr, vel, force, mass, dt, fixed, steps, status


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _md_state(steps, status):
    from matdeeplearn_amd import ops
    state = ops.md_state(len(steps), dev())
    state.steps.copy_(_t(steps))
    state.status.copy_(_t(status))
    return state


def _bits(a):
    return (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)).view(np.int64)


@pytest.mark.parametrize("with_fixed", [True, False])
def test_onstep_velocity_has_the_bits_of_the_host_reference_in_every_branch(with_fixed):
    from matdeeplearn_amd import ops
    node_ptr, vel, force, mass, dt, fixed, steps, status = _inputs()
    fixed = fixed if with_fixed else None
    N, B = len(mass), len(SIZES)
    sentinel = np.random.default_rng(1).normal(size=(N, 3))
    ref = tvh.onstep_velocity_reference(vel, force, mass, fixed, node_ptr, dt, steps, status, out=sentinel)
    # the reference's own values: every branch is there
    seg = lambda b: slice(node_ptr[b], node_ptr[b + 1])
    assert np.array_equal(ref[seg(STOPPED)], sentinel[seg(STOPPED)]) and np.array_equal(ref[seg(ONE)], vel[seg(ONE)])     # steps == 0: vel
    assert not np.array_equal(ref[seg(BIG)], vel[seg(BIG)]) and (not with_fixed or not ref[seg(ALL_FIXED)].any())
    state = _md_state(steps, status)
    out = _t(sentinel)
    got = ops.md_onstep_velocity(_t(vel), _t(force), _t(mass), _t(node_ptr), state, _t(dt), None if fixed is None else _t(fixed), out)
    assert got is out and np.array_equal(_bits(out), _bits(ref))
    assert np.array_equal(state.steps.cpu().numpy(), steps) and np.array_equal(state.status.cpu().numpy(), status)     # the state is read only
    # a new tensor where none is given (rows nobody writes are zero), a cell-mode state, a plain number for dt
    cell_state = ops.md_cell_state(B, dev())
    cell_state.steps.copy_(_t(steps))
    cell_state.status.copy_(_t(status))
    fresh = ops.md_onstep_velocity(_t(vel), _t(force), _t(mass), _t(node_ptr), cell_state, _t(dt), None if fixed is None else _t(fixed))
    want = tvh.onstep_velocity_reference(vel, force, mass, fixed, node_ptr, dt, steps, status)
    assert np.array_equal(_bits(fresh), _bits(want)) and not fresh[node_ptr[STOPPED]:node_ptr[STOPPED + 1]].any()
    plain = ops.md_onstep_velocity(_t(vel), _t(force), _t(mass), _t(node_ptr), state, 0.25)
    assert np.array_equal(_bits(plain), _bits(tvh.onstep_velocity_reference(vel, force, mass, None, node_ptr, np.full(B, 0.25), steps, status)))
    # each structure alone: the same bits
    for b in range(B):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        alone = ops.md_onstep_velocity(_t(vel[a:e]), _t(force[a:e]), _t(mass[a:e]), _t(np.array([0, e - a])), _md_state(steps[b:b + 1], status[b:b + 1]),
                                       _t(dt[b:b + 1]), None if fixed is None else _t(fixed[a:e]), _t(sentinel[a:e]))
        assert np.array_equal(_bits(alone), _bits(ref[a:e])), b


@functools.lru_cache(maxsize=None)
def _vacf_case(T, remove_com, with_fixed):
    """two frames against a ring of four origins, and the reference after each"""
    node_ptr, _, _, mass, _, fixed, _, status = _inputs()
    rng = np.random.default_rng(43 + T)
    N = len(mass)
    types = rng.integers(0, T, N)
    frames = [rng.normal(size=(N, 3)) + rng.normal(size=(1, 3)) for _ in LAGS]       # a centre-of-mass velocity worth removing
    origins = rng.normal(size=(len(LAGS[0]), N, 3)) + rng.normal(size=(len(LAGS[0]), 1, 3))
    fixed = fixed if with_fixed else None
    B = len(SIZES)
    base = (np.zeros((B, 2, T, N_LAGS)), np.zeros((B, N_LAGS), np.int64), np.zeros((B, 2, T, N_LAGS)))
    for b in (EMPTY, STOPPED):                                   # what a skipped structure must keep
        base[0][b], base[1][b] = rng.normal(size=base[0][b].shape), rng.integers(1, 9, N_LAGS)
    refs = [base]
    for v, lag in zip(frames, LAGS):
        refs.append(tvh.vacf_reference(v, origins, lag, mass, types, fixed, node_ptr, status, remove_com, T, N_LAGS, refs[-1]))
    return types, frames, origins, fixed, refs


def _vacf_launch(T, remove_com, types, frames, origins, fixed, mass, node_ptr, status, base):
    from matdeeplearn_amd import ops
    state = ops.vacf_state(types, node_ptr, T, dict(n_lags=N_LAGS, n_origins=len(LAGS[0])), dev())
    state.origins.copy_(_t(origins))
    state.vacf_sum.copy_(_t(base[0]))
    state.vacf_count.copy_(_t(base[1]))
    fixed_t, mass_t, status_t = None if fixed is None else _t(fixed), _t(mass), _t(status)
    for v, lag in zip(frames, LAGS):
        assert ops.vacf_accumulate(_t(v), _t(np.asarray(lag, np.int32)), mass_t, state, fixed_t, status_t, remove_com) is state
    return state


@pytest.mark.parametrize("T,remove_com,with_fixed", [(1, True, True), (1, False, True), (3, True, True), (3, False, True), (5, True, True),
                                                      (5, False, True), (3, True, False)])
def test_vacf_accumulate_matches_the_host_reference_in_every_branch(T, remove_com, with_fixed):
    """On the MI355X: vacf_sum within 7.7e-15 of the sum of the magnitudes of a word's terms at worst (T = 5, centre of mass removed;
    2.5e-16 ... 7.7e-16 in the other six cases; bound 1e-12); counts exact."""
    node_ptr, _, _, mass, _, _, _, status = _inputs()
    types, frames, origins, fixed, refs = _vacf_case(T, remove_com, with_fixed)
    B = len(SIZES)
    ref_sum, ref_count, ref_abs = refs[-1]
    # the reference's own values: every role is there
    want = np.zeros((B, N_LAGS), np.int64)
    want[:, [0, N_LAGS - 1]] += 1                              # the first launch: lag 0 and the last lag (one slot empty, one past the end)
    want[:, [2, 0, 1]] += 1                                    # the second
    want[[EMPTY, STOPPED]] = refs[0][1][[EMPTY, STOPPED]]
    assert np.array_equal(ref_count, want) and np.array_equal(ref_sum[[EMPTY, STOPPED]], refs[0][0][[EMPTY, STOPPED]])
    running = [b for b in range(B) if b not in (EMPTY, STOPPED)]
    assert not ref_sum[running][:, :, :, 3].any()              # no slot was at lag 3
    assert with_fixed == (not ref_abs[ALL_FIXED].any()) and (ref_abs[BIG][:, :, 0] > 0).all()
    state = _vacf_launch(T, remove_com, types, frames, origins, fixed, mass, node_ptr, status, refs[0])
    got = state.vacf_sum.cpu().numpy()
    assert np.array_equal(state.vacf_count.cpu().numpy(), ref_count)
    err = np.abs(got - ref_sum)
    worst = float((err[ref_abs > 0] / ref_abs[ref_abs > 0]).max())
    print("vacf_sum (T %d, remove_com %s, fixed %s): largest error %.3e of the sum of the magnitudes of a word's terms (bound 1e-12)"
          % (T, remove_com, with_fixed, worst))
    assert (err <= 1e-12 * ref_abs).all(), worst               # (a word without terms is exactly what it was)
    assert np.array_equal(_bits(got[[EMPTY, STOPPED]]), _bits(refs[0][0][[EMPTY, STOPPED]]))
    # the same inputs again: the same bits
    again = _vacf_launch(T, remove_com, types, frames, origins, fixed, mass, node_ptr, status, refs[0])
    assert torch.equal(again.vacf_sum, state.vacf_sum) and torch.equal(again.vacf_count, state.vacf_count)
    # each structure alone: the bits it has in the batch
    for b in range(B):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        alone = _vacf_launch(T, remove_com, types[a:e], [v[a:e] for v in frames], origins[:, a:e], None if fixed is None else fixed[a:e], mass[a:e],
                             np.array([0, e - a]), status[b:b + 1], tuple(x[b:b + 1] for x in refs[0]))
        assert torch.equal(alone.vacf_sum, state.vacf_sum[b:b + 1]) and torch.equal(alone.vacf_count, state.vacf_count[b:b + 1]), b


def test_dynamics_ops_reject_bad_arguments_on_the_device():
    from matdeeplearn_amd import _lib, ops
    node_ptr, vel, force, mass, dt, fixed, steps, status = [_t(a) for a in _inputs()]
    N, B = mass.shape[0], len(SIZES)
    state = _md_state(steps.cpu().numpy(), status.cpu().numpy())
    for bad in (dict(vel=vel.cpu()), dict(force=force.cpu()), dict(dt=dt.cpu()), dict(vel=vel[:-1]), dict(force=force.double()), dict(mass=mass.float()),
                dict(node_ptr=node_ptr[:-1]), dict(dt=dt[:-1]), dict(fixed=fixed.int()), dict(out=torch.zeros(N, 3, device=dev())),
                dict(out=torch.zeros(N, 3, dtype=torch.float64)), dict(state=None), dict(state=ops.md_state(B, "cpu"))):
        a = dict(dict(vel=vel, force=force, mass=mass, node_ptr=node_ptr, state=state, dt=dt, fixed=fixed, out=None), **bad)
        with pytest.raises(ops.MdlError):
            ops.md_onstep_velocity(a["vel"], a["force"], a["mass"], a["node_ptr"], a["state"], a["dt"], a["fixed"], a["out"])
    types = torch.zeros(N, dtype=torch.int64)
    vstate = ops.vacf_state(types, node_ptr, 1, dict(n_lags=3, n_origins=2), dev())
    lag = torch.tensor([0, -1], dtype=torch.int32, device=dev())
    for bad in (dict(v=vel.cpu()), dict(v=vel.float()), dict(v=vel[:-1]), dict(lag=lag.cpu()), dict(lag=lag[:-1]), dict(lag=lag.long()),
                dict(mass=mass.cpu()), dict(mass=mass[:-1]), dict(fixed=fixed.int()), dict(status=status.long()), dict(status=status[:-1]),
                dict(status=status.cpu()), dict(state=None)):
        a = dict(dict(v=vel, lag=lag, mass=mass, state=vstate, fixed=fixed, status=status), **bad)
        with pytest.raises(ops.MdlError):
            ops.vacf_accumulate(a["v"], a["lag"], a["mass"], a["state"], a["fixed"], a["status"])
    assert not vstate.vacf_sum.any() and not vstate.vacf_count.any()              # nothing above accumulated anything
    # the library's own checks, none of which launches: the type and slot limits, sizes, null pointers
    lib, none = _lib.lib(), [None] * 8
    for args, text in ((none + [5, 1, 1, 65, 3, 1, None, None, None], "at most 64"), (none + [5, 1, 65536, 1, 3, 1, None, None, None], "at most 65535"),
                       (none + [5, 1, 1, 0, 3, 1, None, None, None], "bad K"), (none + [5, 1, 1, 1, 0, 1, None, None, None], "bad K"),
                       (none + [-1, 1, 1, 1, 1, 1, None, None, None], "bad N"), (none + [5, 1, 1, 1, 1, 1, None, None, None], "null pointer")):
        with pytest.raises(ops.MdlError, match=text):
            _lib.check(lib.mdl_vacf_accumulate(*args), "mdl_vacf_accumulate")
    for args, text in ((none + [-1, 1, None, None], "bad N"), (none + [5, -1, None, None], "bad N"), (none + [5, 1, None, None], "null pointer")):
        with pytest.raises(ops.MdlError, match=text):
            _lib.check(lib.mdl_md_onstep_velocity(*args), "mdl_md_onstep_velocity")
    assert lib.mdl_vacf_accumulate(*(none + [0, 3, 1, 1, 1, 1, None, None, None])) == 0 and lib.mdl_md_onstep_velocity(*(none + [5, 0, None, None])) == 0
    z = lambda *s, dtype=torch.float64: torch.zeros(*s, dtype=dtype, device=dev())
    empty = ops.vacf_state(z(0, dtype=torch.int64), z(1, dtype=torch.int64), 1, dict(n_lags=2), device=dev())
    ops.vacf_accumulate(z(0, 3), z(2, dtype=torch.int32), z(0), empty)                               # B = 0: no launch
    assert tuple(ops.md_onstep_velocity(z(0, 3), z(0, 3, dtype=torch.float32), z(0), z(1, dtype=torch.int64), ops.md_state(0, dev()), 1.0).shape) == (0, 3)


# ---------------------------------------------------------------------------------------------
# forces.sample with a forces.Correlate
# ---------------------------------------------------------------------------------------------
STEPS, HOT = 12, tgo.HOT
VACF = dict(n_lags=4, origin_every=2)


def _replay(obs, types, node_ptr, request, steps, mass, fixed, stopped=None):
    """the stored on-step velocities through ops.vacf_accumulate on the schedule the request states; stopped: (structure, step) —
    its status is 2 at every later step"""
    from matdeeplearn_amd import ops
    d = dev()
    B = len(node_ptr) - 1
    state = ops.vacf_state(types, node_ptr, 3, request.vacf, d)
    its = list(range(request.skip, steps + 1, request.every))
    slot, lag = ops.msd_schedule(len(its), request.vacf["n_lags"], request.vacf["origin_every"], request.vacf["n_origins"])
    mass, fixed = _t(mass), _t(fixed.astype(np.uint8))
    for s, it in enumerate(its):
        assert int(obs.frames_step[it]) == it
        v = obs.frames_vel[it].contiguous()
        status = torch.zeros(B, dtype=torch.int32, device=d)
        if stopped is not None and it > stopped[1]:
            status[stopped[0]] = 2
        if slot[s] >= 0:
            state.origins[int(slot[s])].copy_(v)
        ops.vacf_accumulate(v, lag[s].to(d), mass, state, fixed, status, request.vacf["remove_com"])
    return state


def test_sample_with_a_correlate_is_md_to_the_bit_and_its_velocities_are_the_integrators():
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    model, masses, B = tgm._oracle_model(), tmh.md_masses(case), len(case.structs)
    node_ptr, types = case.p["node_ptr"], tgo._types(case)
    args = tgo._run_args(case)
    fixed = args["fixed"]
    # the velocities md draws from these arguments: one launch of the same kernel on the same operands
    v0 = ops.md_velocities(_t(masses), _t(node_ptr), args["kT_init"], args["seed"], _t(fixed))
    request = forces.Correlate(every=1, skip=2, rdf=tgo.RDF, msd=tgo.MSD, frames_every=1, types=types, vacf=VACF)
    with ops.deterministic():
        plain = forces.md(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, **args)
        res, obs = forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, request, **args)
        _, obs_plain = forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, STEPS,
                                     forces.Observe(every=1, skip=2, rdf=tgo.RDF, msd=tgo.MSD, frames_every=1, types=types), **args)
    for k, a, b in zip(res._fields, res, plain):
        assert torch.equal(a, b), k
    assert (res.status == 1).all()
    tgo._same_accumulators(obs, obs_plain)                       # what a plain Observe records is what it was
    assert torch.equal(obs.frames_pos, obs_plain.frames_pos) and obs_plain.frames_vel is None and obs_plain.vacf_sum is None
    N = len(masses)
    assert tuple(obs.frames_vel.shape) == (STEPS + 1, N, 3) and tuple(obs.vacf_sum.shape) == (B, 2, 3, 4) and tuple(obs.vacf_count.shape) == (B, 4)
    # the closing call stores exactly the on-step velocity: the reconstruction is the engine's, to the bit; and the first is what went in
    assert torch.equal(obs.frames_vel[-1], res.velocities)
    assert torch.equal(obs.frames_vel[0], v0) and v0.abs().sum() > 0
    assert not torch.equal(obs.frames_vel[1], obs.frames_vel[0])
    # lag l is reached by the samples l .. STEPS - 2 whose origin (every second sample) is l samples back
    assert obs.vacf_count.cpu().tolist() == [[len([s for s in range(l, STEPS - 1) if (s - l) % 2 == 0]) for l in range(4)]] * B
    replayed = _replay(obs, types, node_ptr, request, STEPS, masses, fixed)
    assert torch.equal(replayed.vacf_sum, obs.vacf_sum) and torch.equal(replayed.vacf_count, obs.vacf_count)
    # the helpers on the device tensors
    c, (freq, dos) = obs.vacf(0), obs.vdos(0)
    assert tuple(c.shape) == (B, 4) and tuple(freq.shape) == tuple(dos.shape) == (B, 4) and tuple(obs.diffusion_gk(0, 4).shape) == (B,)
    has = torch.from_numpy((obs.type_counts[:, 0] > 0).cpu().numpy()).to(dev())
    assert (c[has][:, 0] > 0).all() and torch.isfinite(dos[has]).all()

    # the guard mid-run: a max_disp between two records of the hot structure's largest step, as tests/test_gpu_observe.py places it
    frames = obs.frames_pos.cpu().numpy()
    step = np.sqrt(((frames[1:] - frames[:-1]) ** 2).sum(2))
    largest = np.array([[step[it, a:e].max() for a, e in zip(node_ptr[:-1], node_ptr[1:])] for it in range(STEPS)])
    hot = largest[:, HOT]
    records = [it for it in range(3, STEPS - 3) if hot[it] > 1.05 * hot[:it].max()]
    assert records, hot
    k = records[0]
    max_disp = 0.5 * (hot[k] + hot[:k].max())
    assert max_disp > 2.0 * np.delete(largest, HOT, 1).max()
    with ops.deterministic():
        res2, obs2 = forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, request, **dict(args, max_disp=max_disp))
    want_status, want_steps = [1] * B, [STEPS] * B
    want_status[HOT], want_steps[HOT] = 2, k
    assert res2.status.cpu().tolist() == want_status and res2.steps.cpu().tolist() == want_steps
    # it was correlated at steps 2 .. k and not after; the velocity the integrator left it with is the on-step velocity of step k
    assert int(obs2.vacf_count[HOT, 0]) == len(range(2, k + 1, 2)) < int(obs2.vacf_count[0, 0]) == len(range(2, STEPS + 1, 2))
    assert torch.equal(obs2.frames_vel[:k + 1], obs.frames_vel[:k + 1]) and torch.equal(obs2.frames_vel[-1], res2.velocities)
    a, e = int(node_ptr[HOT]), int(node_ptr[HOT + 1])
    assert torch.equal(obs2.frames_vel[k, a:e], res2.velocities[a:e])
    replayed = _replay(obs2, types, node_ptr, request, STEPS, masses, fixed, stopped=(HOT, k))
    assert torch.equal(replayed.vacf_sum, obs2.vacf_sum) and torch.equal(replayed.vacf_count, obs2.vacf_count)


def test_sample_with_a_correlate_under_npt_is_md_npt_to_the_bit():
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    n = int(case.p["node_ptr"][1])
    model, masses, structs = tgm._oracle_model(), tmh.md_masses(case)[:n], case.structs[:1]
    fixed = np.zeros(n, bool)
    fixed[::5] = True
    npt = dict(pressure=3e-5, tau_p=1.0, compressibility=30.0, max_strain=0.03)
    args = dict(kT=2e-5, seed=11, fixed=fixed)
    types = tgo._types(case)[:n]
    request = forces.Correlate(every=1, skip=2, rdf=tgo.RDF, msd=tgo.MSD, frames_every=1, types=types, vacf=VACF)
    with ops.deterministic():
        plain = forces.md_npt(model, structs, DIST_RANGE, masses, 1.0, STEPS, **npt, **args)
        res, obs = forces.sample(model, structs, DIST_RANGE, masses, 1.0, STEPS, request, npt=npt, **args)
    assert isinstance(res, forces.NPTResult)
    for k, a, b in zip(res._fields, res, plain):
        assert torch.equal(a, b), k
    assert (res.status == 1).all() and not torch.equal(obs.frames_cell[1], obs.frames_cell[0])          # the barostat acted
    assert torch.equal(obs.frames_vel[-1], res.velocities)
    replayed = _replay(obs, types, case.p["node_ptr"][:2], request, STEPS, masses, fixed)
    assert torch.equal(replayed.vacf_sum, obs.vacf_sum) and torch.equal(replayed.vacf_count, obs.vacf_count)


def test_half_the_mass_weighted_lag_zero_sum_is_the_integrators_kinetic_energy():
    """On the MI355X: 1.7e-16 relative at worst over the six structures (bound 1e-12)."""
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    model, masses = tgm._oracle_model(), tmh.md_masses(case)
    request = forces.Correlate(every=1, types=tgo._types(case), vacf=dict(n_lags=1, origin_every=1, remove_com=False))
    with ops.deterministic():
        res, obs = forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, request, **tgo._run_args(case))
    assert (res.status == 1).all() and (obs.vacf_count == STEPS + 1).all() and obs.frames_vel is None
    half = 0.5 * obs.vacf_sum[:, 1, :, 0].sum(1)
    total = res.ekin_trace.sum(0)
    rel = ((half - total).abs() / total).cpu().numpy()
    print("half the mass-weighted lag-0 sum against the sum of ekin_trace: %.3e relative at worst (bound 1e-12)" % rel.max())
    assert (rel <= 1e-12).all(), rel


def test_sample_launches_the_velocity_kernels_once_per_sampled_step_and_never_otherwise():
    from matdeeplearn_amd import forces
    case = trh.cgcnn_case()
    model, masses = tgm._oracle_model(), tmh.md_masses(case)
    steps, every, skip, frames_every = 9, 3, 2, 4
    new = ("mdl_md_onstep_velocity", "mdl_vacf_accumulate")
    request = forces.Correlate(every=every, skip=skip, rdf=tgo.RDF, msd=tgo.MSD, frames_every=frames_every, types=tgo._types(case), vacf=VACF)
    forces.md(model, case.structs, DIST_RANGE, masses, 1.0, 1, **tgo._run_args(case))     # (what a model asks the library once stays out of the lists)
    names = tgl.record(lambda: forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, steps, request, **tgo._run_args(case)))
    segments, current = [], []
    for name in names:                                          # what the loop called in front of every integrator launch
        current.append(name)
        if name == "mdl_md_step":
            segments.append(current)
            current = []
    assert len(segments) == steps + 1 and not set(new) & set(current)
    for it, seg in enumerate(segments):
        sampled, frame = it >= skip and (it - skip) % every == 0, it % frames_every == 0
        assert seg.count(new[0]) == (1 if sampled or frame else 0) and seg.count(new[1]) == (1 if sampled else 0), (it, seg)
        assert seg.count("mdl_msd_accumulate") == (1 if sampled else 0)
        if sampled:                                             # between the evaluation and the integrator launch, in this order
            assert seg[-3:] == [new[0], new[1], "mdl_md_step"], (it, seg[-4:])
    assert [it for it, seg in enumerate(segments) if new[0] in seg and new[1] not in seg] == [0, 4]         # the frame-only steps
    plain = tgl.record(lambda: forces.md(model, case.structs, DIST_RANGE, masses, 1.0, steps, **tgo._run_args(case)))
    assert [n for n in names if n not in new + ("mdl_rdf_accumulate", "mdl_msd_accumulate")] == plain
    observe = forces.Observe(every=every, skip=skip, rdf=tgo.RDF, msd=tgo.MSD, frames_every=frames_every, types=tgo._types(case))
    old = tgl.record(lambda: forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, steps, observe, **tgo._run_args(case)))
    assert not set(new) & set(old) and old == [n for n in names if n not in new]
