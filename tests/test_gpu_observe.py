"""GPU checks of the trajectory observables: the pair-histogram and displacement kernels of csrc/observe.hip (ops.rdf_accumulate,
ops.msd_accumulate) against the fp64 restatements that tests/test_observe_host.py owns — every branch in one launch, exact integers,
the same bits alone and in a batch —, and forces.sample end to end on the oracle CGCNN of tests/test_gpu_md.py: the run is md's /
md_npt's to the bit, and the stored frames replayed through the two ops give the accumulators back bit for bit.

Figures measured on the MI355X are in the docstrings of the tests.  Cost of sampling EVERY step (tools/bench_md.py --observe --steps 80
--repeats 3: every = 1, rdf 256 bins to 8 A, msd 64 lags, three types; CGCNN dim 64; one run on one box): a step of 64 structures /
1,645 atoms takes 3.052 ms without and 3.187 ms with sampling (+0.135 ms), one of 1024 structures / 24,889 atoms 6.791 ms without and
7.273 ms with (+0.482 ms); the integrator launch beside it is 0.013 / 0.016 ms, the force evaluation 2.76 / 6.44 ms (DESIGN.md,
"Trajectory observables")."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_launch_sequence as tgl
import test_gpu_md as tgm
import test_md_host as tmh
import test_observe_host as toh
import test_relax_host as trh
from test_gpu_forces import DIST_RANGE, dev

pytestmark = pytest.mark.gpu

# one atom, a pair, a wave - 1, exactly one wave, a wave + 1, empty, a tile of 256 + 1, two tiles + 1, and what the other roles need
SIZES = [1, 2, 63, 64, 65, 0, 257, 513, 5, 7, 9, 11]
SHELLS, DRIFTED, CLUSTER, SLAB, TRICLINIC, EMPTY, ORTHO, BIG, STOPPED, FLAT, THIN, WIRE = range(12)
R_MAX, NBINS = 5.0, 40
COUNTED = [SHELLS, DRIFTED, CLUSTER, SLAB, TRICLINIC, ORTHO, BIG, WIRE]


def _rdf_inputs(seed):
    """seeded inputs that put every branch of the histogram into one launch (the roles above, by structure)"""
    rng = np.random.default_rng(seed)
    node_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    N, B = int(node_ptr[-1]), len(SIZES)
    seg = lambda b: slice(node_ptr[b], node_ptr[b + 1])
    skewed = lambda a, s: a * np.eye(3) + rng.uniform(-s, s, (3, 3))
    cell, pbc, pos = np.zeros((B, 3, 3)), np.full(B, 7, np.int32), np.zeros((N, 3))
    cell[SHELLS] = skewed(2.1, 0.3)                               # heights below r_max / 2: several shells of images
    cell[DRIFTED] = skewed(3.0, 0.8)
    cell[SLAB] = [[9.0, 0.5, 0.0], [-1.0, 8.0, 0.0], [0.0, 0.0, 0.0]]       # no vacuum row
    cell[TRICLINIC] = skewed(7.0, 1.5)
    cell[ORTHO] = np.diag([11.0, 12.0, 13.0])
    cell[BIG] = skewed(14.0, 2.0)
    cell[STOPPED] = np.eye(3) * 5.0
    cell[FLAT] = [[4.0, 0.0, 0.0], [0.0, 4.0, 0.0], [0.0, 0.0, 0.0]]        # periodic along an axis without extent
    cell[THIN] = np.diag([0.25, 6.0, 6.0])                        # r_max / h = 20 images along x: over the cap of 16
    cell[WIRE] = [[0.0, 0.0, 0.0], [0.0, 0.0, 0.0], [0.3, -0.2, 4.0]]
    pbc[CLUSTER], pbc[SLAB], pbc[WIRE] = 0, 3, 4
    for b in range(B):
        frac = rng.uniform(0.0, 1.0, (SIZES[b], 3))
        if b == CLUSTER:
            pos[seg(b)] = frac * 10.0
        elif b == SLAB:
            pos[seg(b)] = frac[:, :2] @ cell[b][:2] + np.outer(frac[:, 2], [0.0, 0.0, 6.0])
        elif b == WIRE:
            pos[seg(b)] = np.outer(frac[:, 2], cell[b][2]) + np.c_[frac[:, :2] * 5.0, np.zeros(SIZES[b])]
        else:
            pos[seg(b)] = frac @ cell[b]
    # unwrapped coordinates: whole lattice vectors added, many of them
    pos[seg(DRIFTED)] += rng.integers(-50, 51, (2, 3)) @ cell[DRIFTED]
    pos[seg(ORTHO)][::7] += rng.integers(-3, 4, (len(pos[seg(ORTHO)][::7]), 3)) @ cell[ORTHO]
    pos[seg(WIRE)][::2] += np.outer(rng.integers(-9, 10, len(pos[seg(WIRE)][::2])), cell[WIRE][2])
    pos[seg(SHELLS)] += np.array([7, -4, 12]) @ cell[SHELLS]
    status = np.zeros(B, np.int32)
    status[STOPPED] = 2
    types = rng.integers(0, 3, N)
    return pos, types, node_ptr, cell, pbc, status


@functools.lru_cache(maxsize=None)
def _rdf_case():
    """the inputs and their reference (T = 3), re-seeded here on the CPU until no decision is marginal: no counted distance
    within 1e-9 of a bin edge or of r_max, no image count within 1e-3 of the cap"""
    for seed in range(31, 41):
        inp = _rdf_inputs(seed)
        ref, dists, ratios = toh.rdf_reference(*inp, R_MAX, NBINS, 3)
        u = dists * (NBINS / R_MAX)
        margin = min(np.abs(u - np.rint(u)).min() * (R_MAX / NBINS), (R_MAX - dists).min())
        if margin > 1e-9 and (np.abs(ratios - toh.MAX_IMAGES) > 1e-3).all():
            return inp, ref, dists, ratios, margin
    raise AssertionError("no seed without a marginal pair")


def _rdf_launch(inp, T, state=None):
    from matdeeplearn_amd import ops
    pos, types, node_ptr, cell, pbc, status = inp
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    if state is None:
        state = ops.observe_state(types if T > 1 else np.zeros_like(types), node_ptr, T, rdf=dict(r_max=R_MAX, nbins=NBINS), device=dev())
    assert ops.rdf_accumulate(t(pos), t(cell), t(pbc), state, t(status)) is state
    return state


@pytest.mark.parametrize("T", [3, 1])
def test_rdf_accumulate_matches_the_host_reference_in_every_branch(T):
    """On the MI355X: 83 810 counted pairs, the nearest 2.0e-7 A from a bin edge or r_max; hist, frames and flag are the reference's
    integers, vol_sum within 1e-12."""
    inp, ref, dists, ratios, margin = _rdf_case()
    pos, types, node_ptr, cell, pbc, status = inp
    B = len(SIZES)
    # the reference's own values: every role is there
    assert ref["flag"].tolist() == [0] * 9 + [toh.NO_VOLUME, toh.TOO_MANY_IMAGES, 0]
    assert ref["frames"].tolist() == [1 if b in COUNTED else 0 for b in range(B)]
    assert ratios[SHELLS] > 2.0 and ratios[THIN] == 20.0 and ratios[BIG] < 1.0
    assert all(ref["hist"][b].sum() > 0 for b in COUNTED) and not any(ref["hist"][b].any() for b in range(B) if b not in COUNTED)
    assert ref["vol_sum"][CLUSTER] == 0.0 and ref["vol_sum"][SLAB] == 0.0 and ref["vol_sum"][BIG] > 1000.0
    print("%d counted pairs, the nearest %.1e A from a bin edge or r_max" % (len(dists), margin))
    if T == 1:                                                  # one type: the same pairs in one histogram
        ref = dict(ref, hist=ref["hist"].sum(1, keepdims=True))
    state = _rdf_launch(inp, T)
    for k in ("hist", "frames", "flag"):
        assert np.array_equal(getattr(state, k).cpu().numpy(), ref[k]), k
    vol = state.vol_sum.cpu().numpy()
    assert (np.abs(vol - ref["vol_sum"]) <= 1e-12 * ref["vol_sum"]).all(), (vol, ref["vol_sum"])
    # a second launch on the same accumulators doubles them
    _rdf_launch(inp, T, state)
    assert np.array_equal(state.hist.cpu().numpy(), 2 * ref["hist"]) and np.array_equal(state.frames.cpu().numpy(), 2 * ref["frames"])
    assert np.array_equal(state.flag.cpu().numpy(), ref["flag"]) and (np.abs(state.vol_sum.cpu().numpy() - 2 * ref["vol_sum"]) <= 2e-12 * ref["vol_sum"]).all()


def test_rdf_accumulate_gives_every_structure_its_integers_alone():
    inp, ref, _, _, _ = _rdf_case()
    pos, types, node_ptr, cell, pbc, status = inp
    for b in range(len(SIZES)):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        alone = _rdf_launch((pos[a:e], types[a:e], np.array([0, e - a]), cell[b:b + 1], pbc[b:b + 1], status[b:b + 1]), 3)
        for k in ("hist", "frames", "flag"):
            assert np.array_equal(getattr(alone, k).cpu().numpy(), ref[k][b:b + 1]), (b, k)


def test_observe_ops_reject_bad_arguments_on_the_device():
    from matdeeplearn_amd import ops
    inp = _rdf_case()[0]
    pos, types, node_ptr, cell, pbc, status = [torch.from_numpy(np.ascontiguousarray(a)).to(dev()) for a in inp]
    N = pos.shape[0]
    state = ops.observe_state(types, node_ptr, 3, rdf=dict(r_max=R_MAX, nbins=NBINS), msd=dict(n_lags=4, origin_every=1), device=dev())
    mass, lag = torch.ones(N, dtype=torch.float64, device=dev()), torch.tensor([0, -1, -1, -1], dtype=torch.int32, device=dev())
    for bad in (dict(pos=pos[:-1]), dict(pos=pos.float()), dict(cell=cell[:-1]), dict(cell=cell.float()), dict(pbc=pbc.long()),
                dict(status=status.long()), dict(status=status[:-1]), dict(pos=pos.cpu()), dict(state=None)):
        a = dict(dict(pos=pos, cell=cell, pbc=pbc, state=state, status=status), **bad)
        with pytest.raises(ops.MdlError):
            ops.rdf_accumulate(a["pos"], a["cell"], a["pbc"], a["state"], a["status"])
    for bad in (dict(lag=lag[:-1]), dict(lag=lag.long()), dict(lag=lag.cpu()), dict(mass=mass.float()), dict(mass=mass[:-1]),
                dict(fixed=torch.zeros(N, dtype=torch.int32, device=dev())), dict(pos=pos[:-1])):
        a = dict(dict(pos=pos, lag=lag, mass=mass, fixed=None), **bad)
        with pytest.raises(ops.MdlError):
            ops.msd_accumulate(a["pos"], a["lag"], a["mass"], state, a["fixed"], status)
    with pytest.raises(ops.MdlError, match=r"types must be in 0 \.\. 1"):                            # a device tensor is read once, here
        ops.observe_state(types, node_ptr, 2, rdf=dict(r_max=R_MAX, nbins=NBINS))
    assert not state.hist.any() and not state.frames.any() and not state.msd_count.any()            # nothing above counted anything
    z = lambda *s, dtype=torch.float64: torch.zeros(*s, dtype=dtype, device=dev())
    empty = ops.observe_state(z(0, dtype=torch.int64), z(1, dtype=torch.int64), 1, rdf=dict(r_max=1.0, nbins=4), msd=dict(n_lags=2), device=dev())
    ops.rdf_accumulate(z(0, 3), z(0, 3, 3), z(0, dtype=torch.int32), empty)                         # B = 0: no launch
    ops.msd_accumulate(z(0, 3), z(2, dtype=torch.int32), z(0), empty)


# ---------------------------------------------------------------------------------------------
# MSD
# ---------------------------------------------------------------------------------------------
MSD_T, MSD_LAGS = 5, 5                                           # five types: a full reduction of four and a partial one
MSD_LAG = [-1, 0, MSD_LAGS - 1, 2]                               # an empty slot, the origin just stored, the last lag, one between


@functools.lru_cache(maxsize=None)
def _msd_case():
    rng = np.random.default_rng(23)
    node_ptr = np.concatenate([[0], np.cumsum(SIZES)]).astype(np.int64)
    N, B = int(node_ptr[-1]), len(SIZES)
    pos = rng.uniform(0.0, 10.0, (N, 3))
    origins = pos[None] + rng.normal(size=(len(MSD_LAG), N, 3)) * rng.uniform(0.1, 2.0, (len(MSD_LAG), 1, 1)) + rng.normal(size=(len(MSD_LAG), 1, 3))
    origins[1] = pos                                            # lag 0: nothing has moved
    mass, types = rng.uniform(1.0, 20.0, N), rng.integers(0, MSD_T, N)
    fixed = np.zeros(N, np.uint8)
    fixed[node_ptr[TRICLINIC]:node_ptr[TRICLINIC + 1]][::4] = 1
    fixed[node_ptr[BIG]:node_ptr[BIG + 1]][5::9] = 1
    fixed[node_ptr[FLAT]:node_ptr[FLAT + 1]] = 1                  # no free atom at all
    status = np.zeros(B, np.int32)
    status[STOPPED] = 2
    inp = (pos, origins, MSD_LAG, mass, types, fixed, node_ptr, status)
    return inp, {rc: toh.msd_reference(*inp, rc, MSD_T, MSD_LAGS) for rc in (True, False)}


def _msd_launch(inp, remove_com):
    from matdeeplearn_amd import ops
    pos, origins, lag, mass, types, fixed, node_ptr, status = inp
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev())
    state = ops.observe_state(types, node_ptr, MSD_T, msd=dict(n_lags=MSD_LAGS, n_origins=len(lag)), device=dev())
    state.origins.copy_(t(origins))
    ops.msd_accumulate(t(pos), t(np.asarray(lag, np.int32)), t(mass), state, t(fixed), t(status), remove_com)
    return state


@pytest.mark.parametrize("remove_com", [True, False])
def test_msd_accumulate_matches_the_host_reference(remove_com):
    """On the MI355X: msd_sum within 3.2e-16 (centre of mass removed) and 1.7e-16 (kept) of a structure's largest magnitude at
    worst (bound 1e-12); counts exact."""
    inp, refs = _msd_case()
    node_ptr = inp[6]
    ref_sum, ref_count = refs[remove_com]
    B = len(SIZES)
    want = np.zeros((B, MSD_LAGS), np.int64)
    want[:, [0, 2, MSD_LAGS - 1]] = 1
    want[[EMPTY, STOPPED]] = 0
    assert np.array_equal(ref_count, want) and not ref_sum[:, :, 0].any() and not ref_sum[FLAT].any() and (ref_sum[BIG][:, 2] > 0).all()
    assert not np.allclose(refs[True][0], refs[False][0])         # the centre of mass has moved
    state = _msd_launch(inp, remove_com)
    assert np.array_equal(state.msd_count.cpu().numpy(), ref_count)
    tgm._close(state.msd_sum.view(B, -1), ref_sum.reshape(B, -1), np.arange(B + 1), "msd_sum (remove_com %s)" % remove_com)
    assert not state.msd_sum[:, :, 0].any()                      # lag 0 is exactly zero
    again = _msd_launch(inp, remove_com)
    assert torch.equal(again.msd_sum, state.msd_sum) and torch.equal(again.msd_count, state.msd_count)
    # each structure alone: the same bits
    pos, origins, lag, mass, types, fixed, _, status = inp
    for b in range(B):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        alone = _msd_launch((pos[a:e], origins[:, a:e], lag, mass[a:e], types[a:e], fixed[a:e], np.array([0, e - a]), status[b:b + 1]), remove_com)
        assert torch.equal(alone.msd_sum, state.msd_sum[b:b + 1]) and torch.equal(alone.msd_count, state.msd_count[b:b + 1]), b


# ---------------------------------------------------------------------------------------------
# forces.sample
# ---------------------------------------------------------------------------------------------
STEPS, HOT = 20, 1
RDF, MSD = dict(r_max=6.0, nbins=64), dict(n_lags=6, origin_every=2)


def _run_args(case, **kw):
    """Langevin dynamics of the six structures of the oracle case, one of them (HOT) in a bath a thousand times hotter than the
    velocities it starts with: its steps grow along the run, the manner in which a guard comes to act mid-run"""
    B, N = len(case.structs), len(case.p["pos"])
    kT = np.full(B, 2e-5)
    kT[HOT] = 2e-2
    fixed = np.zeros(N, bool)
    fixed[::5] = True
    return dict(dict(kT=kT, gamma=0.05, kT_init=2e-5, seed=3, fixed=fixed, max_disp=10.0), **kw)


def _types(case):
    return np.asarray(case.p["numbers"]) % 3


def _replay(obs, case, request, mass, fixed, cells=None, stopped=None):
    """the stored frames through ops.rdf_accumulate / ops.msd_accumulate on the schedule the request states; stopped: (structure,
    step) — its status is 2 at every later step"""
    from matdeeplearn_amd import ops
    d = dev()
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(d)
    B = len(case.p["node_ptr"]) - 1 if cells is None else cells.shape[1]
    node_ptr = case.p["node_ptr"][:B + 1]
    N = int(node_ptr[-1])
    msd = dict(request.msd)
    state = ops.observe_state(_types(case)[:N], node_ptr, 3, request.rdf, msd, d)
    its = list(range(request.skip, STEPS + 1, request.every))
    slot, lag = ops.msd_schedule(len(its), msd["n_lags"], msd["origin_every"], msd["n_origins"])
    pbc, cell0, mass, fixed = t(np.asarray(case.p["pbc"], np.int32)[:B]), t(case.p["cell"][:B]), t(mass[:N]), t(fixed[:N].astype(np.uint8))
    for s, it in enumerate(its):
        assert int(obs.frames_step[it]) == it
        pos = obs.frames_pos[it].contiguous()
        status = torch.zeros(B, dtype=torch.int32, device=d)
        if stopped is not None and it > stopped[1]:
            status[stopped[0]] = 2
        ops.rdf_accumulate(pos, cell0 if cells is None else cells[it].contiguous(), pbc, state, status)
        if slot[s] >= 0:
            state.origins[int(slot[s])].copy_(pos)
        ops.msd_accumulate(pos, lag[s].to(d), mass, state, fixed, status, msd["remove_com"])
    return state


def _same_accumulators(obs, state):
    for k in ("hist", "frames", "flag", "vol_sum", "msd_sum", "msd_count"):
        assert torch.equal(getattr(obs, k), getattr(state, k)), k


def test_sample_is_md_to_the_bit_and_its_frames_replay_to_its_accumulators():
    """On the MI355X: the hot structure's largest step grows from 0.04 A to 0.33 A over the first eight steps; the guard placed
    between two of its records (0.154 and 0.207 A) stops it at step 3, after which its frames and msd counts stay behind those of
    the others."""
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    model, masses, B = tgm._oracle_model(), tmh.md_masses(case), len(case.structs)
    node_ptr = case.p["node_ptr"]
    args = _run_args(case)
    request = forces.Observe(every=1, skip=2, rdf=RDF, msd=MSD, frames_every=1, types=_types(case))
    with ops.deterministic():
        plain = forces.md(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, **args)
        res, obs = forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, request, **args)
    assert isinstance(res, forces.MDResult) and isinstance(obs, forces.Observations)
    for k, a, b in zip(res._fields, res, plain):
        assert torch.equal(a, b), k
    assert (res.status == 1).all() and obs.species is None and obs.frames_cell is None
    assert tuple(obs.hist.shape) == (B, 6, 64) and tuple(obs.msd_sum.shape) == (B, 3, 6) and tuple(obs.frames_pos.shape) == (STEPS + 1,) + tuple(res.positions.shape)
    assert obs.frames_step.cpu().tolist() == list(range(STEPS + 1)) and torch.equal(obs.frames_pos[-1], res.positions)
    assert np.array_equal(obs.frames_pos[0].cpu().numpy(), case.p["pos"])
    assert (obs.frames == STEPS + 1 - 2).all() and (obs.flag == 0).all() and (obs.hist.sum((1, 2)) > 0).all()
    # lag l is reached by the samples l .. 18 whose origin (every second sample) is l samples back
    assert obs.msd_count.cpu().tolist() == [[len([s for s in range(l, STEPS - 1) if (s - l) % 2 == 0]) for l in range(6)]] * B
    types, fixed = _types(case), args["fixed"]
    counts = np.array([[((types[a:e] == t) & ~fixed[a:e]).sum() for t in range(3)] for a, e in zip(node_ptr[:-1], node_ptr[1:])])
    assert np.array_equal(obs.type_counts.cpu().numpy(), counts) and (obs.type_totals.sum(1).cpu().numpy() == np.diff(node_ptr)).all()
    _same_accumulators(obs, _replay(obs, case, request, masses, fixed))
    # the helpers on the device tensors: shapes, and an msd that grows with the lag
    g, msd = obs.g(0, 1), obs.msd(0)
    assert tuple(g.shape) == (B, 64) and tuple(obs.r().shape) == (64,) and tuple(msd.shape) == (B, 6) and tuple(obs.diffusion(0, 1, 6).shape) == (B,)
    assert (msd[HOT, 1:] > msd[HOT, :-1]).all() and (msd[:, 0][torch.from_numpy(counts[:, 0] > 0).to(dev())] == 0).all() and torch.equal(obs.lag_time, torch.ones(B, dtype=torch.float64, device=dev()))

    # the guard mid-run: the largest step of every structure from the stored frames, a max_disp between two records of the hot one
    frames = obs.frames_pos.cpu().numpy()
    step = np.sqrt(((frames[1:] - frames[:-1]) ** 2).sum(2))                                        # [STEPS, N]
    largest = np.array([[step[it, a:e].max() for a, e in zip(node_ptr[:-1], node_ptr[1:])] for it in range(STEPS)])
    hot = largest[:, HOT]
    records = [it for it in range(3, STEPS - 3) if hot[it] > 1.05 * hot[:it].max()]
    print("largest step of the hot structure per step", np.round(hot, 3), "records", records)
    assert records, hot
    k = records[0]
    max_disp = 0.5 * (hot[k] + hot[:k].max())
    assert max_disp > 2.0 * np.delete(largest, HOT, 1).max()      # nobody else comes near it
    with ops.deterministic():
        res2, obs2 = forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, request, **dict(args, max_disp=max_disp))
    want_status, want_steps = [1] * B, [STEPS] * B
    want_status[HOT], want_steps[HOT] = 2, k
    assert res2.status.cpu().tolist() == want_status and res2.steps.cpu().tolist() == want_steps
    assert torch.equal(obs2.frames_pos[:k + 1], obs.frames_pos[:k + 1]) and torch.equal(obs2.frames_pos[-1], res2.positions)
    # it was sampled at steps 2 .. k and not after
    want_frames = [STEPS - 1] * B
    want_frames[HOT] = k - 1
    assert obs2.frames.cpu().tolist() == want_frames and int(obs2.msd_count[HOT].sum()) < int(obs2.msd_count[0].sum())
    _same_accumulators(obs2, _replay(obs2, case, request, masses, fixed, stopped=(HOT, k)))


def test_sample_under_npt_is_md_npt_to_the_bit_and_samples_the_live_cell():
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    n = int(case.p["node_ptr"][1])
    model, masses, structs = tgm._oracle_model(), tmh.md_masses(case)[:n], case.structs[:1]
    fixed = np.zeros(n, bool)
    fixed[::5] = True
    npt = dict(pressure=3e-5, tau_p=1.0, compressibility=30.0, max_strain=0.03)
    args = dict(kT=2e-5, seed=11, fixed=fixed)
    request = forces.Observe(every=1, skip=2, rdf=RDF, msd=MSD, frames_every=1, types=_types(case)[:n])
    with ops.deterministic():
        plain = forces.md_npt(model, structs, DIST_RANGE, masses, 1.0, STEPS, **npt, **args)
        res, obs = forces.sample(model, structs, DIST_RANGE, masses, 1.0, STEPS, request, npt=npt, **args)
    assert isinstance(res, forces.NPTResult)
    for k, a, b in zip(res._fields, res, plain):
        assert torch.equal(a, b), k
    assert (res.status == 1).all() and tuple(obs.frames_cell.shape) == (STEPS + 1, 1, 3, 3) and torch.equal(obs.frames_cell[-1], res.cell)
    assert np.array_equal(obs.frames_cell[0].cpu().numpy(), case.p["cell"][:1]) and not torch.equal(obs.frames_cell[1], obs.frames_cell[0])
    _same_accumulators(obs, _replay(obs, case, request, masses, fixed, cells=obs.frames_cell))
    # the volume that was summed is that of the live cell, frame by frame
    vol = torch.linalg.det(obs.frames_cell[2:, 0]).abs().sum()
    assert abs(float(obs.vol_sum[0] - vol)) <= 1e-12 * float(vol) and abs(float(obs.vol_sum[0]) - (STEPS - 1) * float(plain.volume_trace[0, 0])) > 1e-6 * float(vol)


def test_sample_launches_each_kernel_once_per_sampled_step_and_never_otherwise():
    from matdeeplearn_amd import forces
    case = trh.cgcnn_case()
    model, masses = tgm._oracle_model(), tmh.md_masses(case)
    steps, every, skip = 9, 3, 2
    request = forces.Observe(every=every, skip=skip, rdf=RDF, msd=MSD, types=_types(case))
    forces.md(model, case.structs, DIST_RANGE, masses, 1.0, 1, **_run_args(case))       # (what a model asks the library once stays out of the lists)
    names = tgl.record(lambda: forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, steps, request, **_run_args(case)))
    segments, current = [], []
    for name in names:                                          # what the loop called in front of every integrator launch
        current.append(name)
        if name == "mdl_md_step":
            segments.append(current)
            current = []
    assert len(segments) == steps + 1 and "mdl_rdf_accumulate" not in current and "mdl_msd_accumulate" not in current
    for it, seg in enumerate(segments):
        want = 1 if it >= skip and (it - skip) % every == 0 else 0
        assert seg.count("mdl_rdf_accumulate") == want and seg.count("mdl_msd_accumulate") == want, (it, seg)
    plain = tgl.record(lambda: forces.md(model, case.structs, DIST_RANGE, masses, 1.0, steps, **_run_args(case)))
    assert [n for n in names if n not in ("mdl_rdf_accumulate", "mdl_msd_accumulate")] == plain
