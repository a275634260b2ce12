"""GPU checks of the reciprocal-space layer: the kernels of csrc/sq.hip (ops.density_modes, ops.sq_accumulate) against the fp64
restatements that tests/test_sq_host.py owns — every branch in one launch, every word of rho within the rounding bound derived there
(density_modes_reference), the products to the bit, the same bits alone and in a batch —, and forces.sample with a forces.Scatter end
to end on the oracle CGCNN of tests/test_gpu_md.py: the run is md's / md_npt's to the bit, what a Correlate records is what it was,
and the stored frames replayed through ops.density_modes / ops.sq_accumulate give every accumulator back bit for bit."""
import functools

import numpy as np
import pytest
import torch

import test_gpu_launch_sequence as tgl
import test_gpu_md as tgm
import test_gpu_observe as tgo
import test_gpu_vacf as tgv
import test_md_host as tmh
import test_relax_host as trh
import test_sq_host as tsh
from test_gpu_forces import DIST_RANGE, dev
from test_sq_host import BAD, BIG, EMPTY, OPEN, SINGULAR, SIZES, STOPPED

pytestmark = pytest.mark.gpu

N_LAGS = 5
LAGS = ([-1, 0, N_LAGS - 1, N_LAGS + 2], [2, 0, -1, 1])         # two launches: an empty slot, lag 0, the last lag, one past the last
SKIPPED = (EMPTY, STOPPED, OPEN, SINGULAR)                       # nothing of them is written but the flag of the last two
HEALED = 2                                                       # the launch from which on the flagged structures would be fine


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev())


def _bits(a):
    return (a.cpu().numpy() if torch.is_tensor(a) else np.asarray(a, np.float64)).view(np.int64)


@functools.lru_cache(maxsize=None)
def _sentinels(T, Q):
    """what the buffers hold in front of the first launch: (rho, frames, cell_sum, flag)"""
    rng, B = np.random.default_rng(11), len(SIZES)
    return rng.normal(size=(B, T, Q, 2)), rng.integers(1, 9, B), rng.normal(size=(B, 9)), np.zeros(B, np.int32)


def _state(T, Q, types, node_ptr, base, fqt=None):
    """a state whose buffers start from `base`; the type outside 0 .. T - 1 is put in behind ops.sq_state's own check of the types"""
    from matdeeplearn_amd import ops
    state = ops.sq_state(np.clip(types, 0, T - 1), node_ptr, T, dict(q=tsh.gpu_inputs()[4][:Q], fqt=fqt), dev())
    state.types.copy_(_t(types.astype(np.int32)))
    for t, a in zip((state.rho, state.frames, state.cell_sum, state.flag), base):
        t.copy_(_t(a))
    return state


def _modes(T, Q, sl=slice(None), launches=1, b0=0, base=None):
    """`launches` launches of mdl_density_modes on the structures b0 + sl of gpu_inputs(): pos, then pos2 with every cell whole and
    every axis periodic"""
    from matdeeplearn_amd import ops
    node_ptr, cell, pbc, status, qvec, pos, pos2 = tsh.gpu_inputs()
    B = len(SIZES)
    idx = np.arange(B)[sl]
    a, e = int(node_ptr[idx[0]]), int(node_ptr[idx[-1] + 1])
    base = _sentinels(T, Q) if base is None else base
    state = _state(T, Q, tsh.gpu_types(T)[a:e], node_ptr[idx[0]:idx[-1] + 2] - a, tuple(x[idx] for x in base))
    healed = np.where(np.arange(B)[:, None, None] == SINGULAR, np.eye(3), cell)
    for k in range(launches):
        first = k == 0
        got = ops.density_modes(_t((pos if first else pos2)[a:e]), _t((cell if first else healed)[idx]), _t(pbc[idx] if first else np.full(len(idx), 7, np.int32)),
                                state, _t(status[idx]))
        assert got is state
    return state


@pytest.mark.parametrize("T", [1, 3, 8])
@pytest.mark.parametrize("Q", [1, 255, 256, 257])
def test_density_modes_is_within_the_derived_bound_of_the_host_reference_in_every_branch(T, Q):
    """On the MI355X (one run): the largest |rho - reference| is 4.1e-14 (T = 1, Q >= 255; 1.8e-14 at T = 3, 8.9e-15 at T = 8), at
    worst 1.0 % of the derived bound (T = 8), whose largest value is 2.7e-10 (513 terms at |phi| up to 70)."""
    from matdeeplearn_amd import ops
    assert T <= ops.SQ_MAX_TYPES == 8
    node_ptr, cell, pbc, status, qvec, pos, pos2 = tsh.gpu_inputs()
    B = len(SIZES)
    base = _sentinels(T, Q)
    ref = tsh.density_modes_reference(pos, tsh.gpu_types(T), node_ptr, cell, pbc, status, qvec[:Q], T, base)
    ref_rho, ref_frames, ref_cell, ref_flag, bound = ref
    counted = [b for b in range(B) if b not in SKIPPED]
    # the reference's own values: every role is there
    assert ref_flag.tolist() == [0] * 10 + [ops.SQ_NOT_PERIODIC, ops.SQ_BAD_TYPE, ops.SQ_NO_VOLUME]
    assert np.array_equal(ref_frames[counted], base[1][counted] + 1) and np.array_equal(ref_frames[list(SKIPPED)], base[1][list(SKIPPED)])
    assert (bound[BIG] > 0).all() and not bound[list(SKIPPED)].any() and bound.max() < 1e-9     # (a type without atoms: rho = 0, bound 0)
    state = _modes(T, Q)
    rho = state.rho.cpu().numpy()
    err = np.abs(rho - ref_rho)
    worst = float((err[bound > 0] / bound[bound > 0]).max())
    print("rho (T %d, Q %d): largest |rho - reference| %.3e, at worst %.4f of the derived bound (largest bound %.3e)" % (T, Q, err.max(), worst, bound.max()))
    assert (err <= bound).all(), worst                          # (a word nobody writes has a bound of 0: it is exactly what it was)
    for b in SKIPPED:
        assert np.array_equal(_bits(rho[b]), _bits(base[0][b])), b
    # frames and the sum of the cells: exact, and a skipped structure's words keep their bits
    assert np.array_equal(state.frames.cpu().numpy(), ref_frames) and np.array_equal(_bits(state.cell_sum), _bits(ref_cell))
    assert np.array_equal(state.flag.cpu().numpy(), ref_flag)
    assert np.array_equal(_bits(ref_cell[list(SKIPPED)]), _bits(base[2][list(SKIPPED)]))
    # the same inputs again: the same bits
    assert torch.equal(_modes(T, Q).rho, state.rho)
    # the flags are sticky: a second launch in which the two flagged structures would be fine leaves them out all the same
    ref2 = tsh.density_modes_reference(pos2, tsh.gpu_types(T), node_ptr, np.where(np.arange(B)[:, None, None] == SINGULAR, np.eye(3), cell),
                                       np.full(B, 7, np.int32), status, qvec[:Q], T, ref[:4])
    two = _modes(T, Q, launches=HEALED)
    rho2 = two.rho.cpu().numpy()
    assert np.array_equal(two.flag.cpu().numpy(), ref_flag) and np.array_equal(two.frames.cpu().numpy(), ref2[1])
    assert np.array_equal(ref2[1][counted], base[1][counted] + 2) and np.array_equal(_bits(two.cell_sum), _bits(ref2[2]))
    assert (np.abs(rho2 - ref2[0]) <= ref2[4]).all()
    for b in SKIPPED:
        assert np.array_equal(_bits(rho2[b]), _bits(base[0][b])), b
    if Q == 257 or T == 3:
        # each structure alone: the bits it has in the batch
        for b in range(B):
            alone = _modes(T, Q, slice(b, b + 1))
            assert torch.equal(alone.rho, state.rho[b:b + 1]) and torch.equal(alone.frames, state.frames[b:b + 1]), b
            assert torch.equal(alone.cell_sum, state.cell_sum[b:b + 1]) and torch.equal(alone.flag, state.flag[b:b + 1]), b


def test_status_none_counts_the_stopped_structure_too():
    from matdeeplearn_amd import ops
    node_ptr, cell, pbc, status, qvec, pos, _ = tsh.gpu_inputs()
    T, Q = 3, 5
    base = tuple(np.zeros_like(x) for x in _sentinels(T, Q))
    ref = tsh.density_modes_reference(pos, tsh.gpu_types(T), node_ptr, cell, pbc, None, qvec[:Q], T)
    state = _state(T, Q, tsh.gpu_types(T), node_ptr, base)
    ops.density_modes(_t(pos), _t(cell), _t(pbc), state)
    assert int(state.frames[STOPPED]) == 1 == ref[1][STOPPED] and (np.abs(state.rho.cpu().numpy() - ref[0]) <= ref[4]).all()


@functools.lru_cache(maxsize=None)
def _accumulate_case(T, Q, K):
    rng, B, P = np.random.default_rng(13 + T), len(SIZES), T * (T + 1) // 2
    origins = rng.normal(size=(K, B, T, Q, 2)) * 5.0
    base = (rng.normal(size=(B, P, Q)), rng.normal(size=(B, P, N_LAGS, Q)), rng.integers(1, 9, (B, N_LAGS)))
    return origins, base


@pytest.mark.parametrize("T,Q", [(1, 1), (3, 257), (8, 256), (3, 255)])
def test_sq_accumulate_has_the_bits_of_the_host_reference_from_the_devices_own_modes(T, Q):
    from matdeeplearn_amd import ops
    node_ptr, cell, pbc, status, qvec, pos, pos2 = tsh.gpu_inputs()
    B, K = len(SIZES), len(LAGS[0])
    origins, base = _accumulate_case(T, Q, K)
    zeros = tuple(np.zeros_like(x) for x in _sentinels(T, Q))

    def run(sl=slice(None)):
        idx = np.arange(B)[sl]
        a, e = int(node_ptr[idx[0]]), int(node_ptr[idx[-1] + 1])
        state = _state(T, Q, tsh.gpu_types(T)[a:e], node_ptr[idx[0]:idx[-1] + 2] - a, tuple(x[idx] for x in zeros), dict(n_lags=N_LAGS, n_origins=K))
        state.origins.copy_(_t(origins[:, idx]))
        for t, x in zip((state.sq_sum, state.fqt_sum, state.fqt_count), base):
            t.copy_(_t(x[idx]))
        rhos = []
        for frame, lag in zip((pos, pos2), LAGS):
            ops.density_modes(_t(frame[a:e]), _t(cell[idx]), _t(pbc[idx]), state, _t(status[idx]))
            rhos.append(state.rho.cpu().numpy())
            assert ops.sq_accumulate(_t(np.asarray(lag, np.int32)), state, _t(status[idx])) is state
        return state, rhos

    state, rhos = run()
    flag = state.flag.cpu().numpy()
    assert flag.tolist() == [0] * 10 + [1, 4, 2]
    ref = base
    for rho, lag in zip(rhos, LAGS):
        ref = tsh.sq_accumulate_reference(rho, origins, lag, flag, status, node_ptr, T, N_LAGS, ref)
    # the reference's own values: every role is there
    want = np.array(base[2])
    want[:, [0, N_LAGS - 1]] += 1
    want[:, [2, 0, 1]] += 1
    want[list(SKIPPED)] = base[2][list(SKIPPED)]
    assert np.array_equal(ref[2], want)
    running = [b for b in range(B) if b not in SKIPPED]
    assert np.array_equal(ref[1][running][:, :, 3], base[1][running][:, :, 3]) and (ref[0][BIG] != base[0][BIG]).all()
    for k in range(3):
        assert np.array_equal(_bits(ref[k][list(SKIPPED)].astype(np.float64)), _bits(np.asarray(base[k])[list(SKIPPED)].astype(np.float64)))
    # the kernel: bit for bit
    assert np.array_equal(_bits(state.sq_sum), _bits(ref[0])) and np.array_equal(_bits(state.fqt_sum), _bits(ref[1]))
    assert np.array_equal(state.fqt_count.cpu().numpy(), ref[2])
    # the same inputs again, and each structure alone: the same bits
    again, _ = run()
    assert torch.equal(again.sq_sum, state.sq_sum) and torch.equal(again.fqt_sum, state.fqt_sum) and torch.equal(again.fqt_count, state.fqt_count)
    for b in range(B):
        alone, _ = run(slice(b, b + 1))
        assert torch.equal(alone.sq_sum, state.sq_sum[b:b + 1]) and torch.equal(alone.fqt_sum, state.fqt_sum[b:b + 1]), b
        assert torch.equal(alone.fqt_count, state.fqt_count[b:b + 1]), b


def test_sq_accumulate_without_a_ring_gives_s_alone():
    from matdeeplearn_amd import ops
    node_ptr, cell, pbc, status, qvec, pos, pos2 = tsh.gpu_inputs()
    T, Q = 3, 257
    state = _state(T, Q, tsh.gpu_types(T), node_ptr, tuple(np.zeros_like(x) for x in _sentinels(T, Q)))
    assert state.fqt_sum is None and state.origins.shape[0] == 0
    ref = None
    for frame in (pos, pos2):
        ops.density_modes(_t(frame), _t(cell), _t(pbc), state, _t(status))
        ops.sq_accumulate(None, state, _t(status))
        ref = tsh.sq_accumulate_reference(state.rho.cpu().numpy(), np.zeros((0,)), [], state.flag.cpu().numpy(), status, node_ptr, T, 1, ref)
    assert np.array_equal(_bits(state.sq_sum), _bits(ref[0])) and not ref[1].any() and not ref[0][list(SKIPPED)].any() and ref[0][BIG].all()
    # S_aa at n = 0 is N_a^2 per frame, exactly
    types = tsh.gpu_types(T)[node_ptr[BIG]:node_ptr[BIG + 1]]
    assert state.sq_sum[BIG, [0, 3, 5], 1].tolist() == [2.0 * float((types == t).sum()) ** 2 for t in range(3)]


def test_scattering_ops_reject_bad_arguments_on_the_device():
    from matdeeplearn_amd import _lib, ops
    node_ptr, cell, pbc, status, qvec, pos, _ = tsh.gpu_inputs()
    N, B = len(pos), len(SIZES)
    types = np.zeros(N, np.int64)
    with pytest.raises(ops.MdlError, match="at most 8 types"):
        ops.sq_state(types, node_ptr, ops.SQ_MAX_TYPES + 1, dict(n_max=1), dev())
    for q in (np.zeros((4, 2), np.int32), np.zeros((4, 3)), np.zeros(3, np.int32)):
        with pytest.raises(ops.MdlError, match=r"q must be a \[Q, 3\] integer array"):
            ops.sq_state(types, node_ptr, 1, dict(q=q), dev())
    state = ops.sq_state(types, node_ptr, 1, dict(n_max=1, fqt=dict(n_lags=3, n_origins=2)), dev())
    pos_t, cell_t, pbc_t, status_t = _t(pos), _t(cell), _t(pbc), _t(status)
    lag = torch.tensor([0, -1], dtype=torch.int32, device=dev())
    for bad in (dict(pos=pos_t.cpu()), dict(pos=pos_t.float()), dict(pos=pos_t[:-1]), dict(cell=cell_t.cpu()), dict(cell=cell_t[:-1]), dict(pbc=pbc_t.long()),
                dict(pbc=pbc_t.cpu()), dict(status=status_t.long()), dict(status=status_t[:-1]), dict(status=status_t.cpu()), dict(state=None)):
        a = dict(dict(pos=pos_t, cell=cell_t, pbc=pbc_t, state=state, status=status_t), **bad)
        with pytest.raises(ops.MdlError):
            ops.density_modes(a["pos"], a["cell"], a["pbc"], a["state"], a["status"])
    for bad in (dict(lag=lag.cpu()), dict(lag=lag[:-1]), dict(lag=lag.long()), dict(lag=None), dict(status=status_t.long()), dict(status=status_t.cpu()),
                dict(state=None)):
        a = dict(dict(lag=lag, state=state, status=status_t), **bad)
        with pytest.raises(ops.MdlError):
            ops.sq_accumulate(a["lag"], a["state"], a["status"])
    state.qvec = state.qvec.long()                              # a wrong dtype of qvec in a state someone has put together by hand
    with pytest.raises(ops.MdlError, match="qvec must be a contiguous"):
        ops.density_modes(pos_t, cell_t, pbc_t, state, status_t)
    state.qvec = state.qvec.int()[:, :2].contiguous()
    with pytest.raises(ops.MdlError, match="qvec must be a contiguous"):
        ops.density_modes(pos_t, cell_t, pbc_t, state, status_t)
    for k in ("rho", "frames", "cell_sum", "flag", "sq_sum", "fqt_sum", "fqt_count"):
        assert not getattr(state, k).any(), k                   # nothing above wrote anything
    # the library's own checks, none of which launches: the type, tile and slot limits, sizes, null pointers
    lib, none = _lib.lib(), [None] * 7
    for args, text in ((none + [5, 1, 4, 9, None, None, None, None, None], "at most 8"), (none + [5, 1, 65535 * 256 + 1, 1, None, None, None, None, None], "q-tiles"),
                       (none + [5, 2 ** 31, 4, 1, None, None, None, None, None], "overflow the grid"), (none + [5, 1, 4, 0, None, None, None, None, None], "bad T"),
                       (none + [-1, 1, 4, 1, None, None, None, None, None], "bad N"), (none + [5, 1, -4, 1, None, None, None, None, None], "bad N"),
                       (none + [5, 1, 4, 1, None, None, None, None, None], "null pointer")):
        with pytest.raises(ops.MdlError, match=text):
            _lib.check(lib.mdl_density_modes(*args), "mdl_density_modes")
    none = [None] * 6
    for args, text in ((none + [5, 1, 1, 9, 4, 3, None, None, None, None], "at most 8"), (none + [5, 1, 65536, 1, 4, 3, None, None, None, None], "at most 65535"),
                       (none + [5, 1, -1, 1, 4, 3, None, None, None, None], "bad K"), (none + [5, 1, 1, 1, 4, 0, None, None, None, None], "bad K"),
                       (none + [5, 1, 0, 1, 4, 1, None, None, None, None], "null pointer")):
        with pytest.raises(ops.MdlError, match=text):
            _lib.check(lib.mdl_sq_accumulate(*args), "mdl_sq_accumulate")
    assert lib.mdl_density_modes(*([None] * 7 + [5, 0, 4, 1, None, None, None, None, None])) == 0                     # B == 0, N == 0, Q == 0: no launch
    assert lib.mdl_density_modes(*([None] * 7 + [0, 3, 4, 1, None, None, None, None, None])) == 0
    assert lib.mdl_density_modes(*([None] * 7 + [5, 3, 0, 1, None, None, None, None, None])) == 0
    assert lib.mdl_sq_accumulate(*([None] * 6 + [5, 3, 2, 1, 0, 3, None, None, None, None])) == 0
    z = lambda *s, dtype=torch.float64: torch.zeros(*s, dtype=dtype, device=dev())
    empty = ops.sq_state(z(0, dtype=torch.int64), z(1, dtype=torch.int64), 1, dict(n_max=1), device=dev())
    ops.density_modes(z(0, 3), z(0, 3, 3), z(0, dtype=torch.int32), empty)
    ops.sq_accumulate(None, empty)


# ---------------------------------------------------------------------------------------------
# forces.sample with a forces.Scatter
# ---------------------------------------------------------------------------------------------
STEPS = 12
QVEC = np.array([[0, 0, 0], [1, 0, 0], [0, -1, 2], [3, 3, -3], [-2, 0, 5]], np.int32)
SQ = dict(q=QVEC, fqt=dict(n_lags=4, origin_every=2))


def _replay(obs, types, node_ptr, request, steps, pbc, cell0, cells=None):
    """the stored frames through ops.density_modes / ops.sq_accumulate on the schedule the request states"""
    from matdeeplearn_amd import ops
    d, fqt = dev(), request.sq["fqt"]
    state = ops.sq_state(types, node_ptr, 3, request.sq, d)
    its = list(range(request.skip, steps + 1, request.every))
    slot, lag = ops.msd_schedule(len(its), fqt["n_lags"], fqt["origin_every"], fqt["n_origins"])
    for s, it in enumerate(its):
        assert int(obs.frames_step[it]) == it
        ops.density_modes(obs.frames_pos[it].contiguous(), cell0 if cells is None else cells[it].contiguous(), pbc, state)
        if slot[s] >= 0:
            state.origins[int(slot[s])].copy_(state.rho)
        ops.sq_accumulate(lag[s].to(d), state)
    return state


def _same_sq(obs, state):
    for k, got in (("sq_sum", obs.sq_sum), ("frames", obs.sq_frames), ("flag", obs.sq_flag), ("cell_sum", obs.cell_sum), ("fqt_sum", obs.fqt_sum),
                   ("fqt_count", obs.fqt_count), ("qvec", obs.qvec)):
        assert torch.equal(got, getattr(state, k)), k


def test_sample_with_a_scatter_is_md_to_the_bit_and_its_frames_replay_to_its_structure_factors():
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    model, masses, B = tgm._oracle_model(), tmh.md_masses(case), len(case.structs)
    node_ptr, types = case.p["node_ptr"], tgo._types(case)
    args = tgo._run_args(case)
    common = dict(every=1, skip=2, rdf=tgo.RDF, msd=tgo.MSD, frames_every=1, types=types, vacf=tgv.VACF)
    request = forces.Scatter(sq=SQ, **common)
    with ops.deterministic():
        plain = forces.md(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, **args)
        res, obs = forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, request, **args)
        _, obs_c = forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, STEPS, forces.Correlate(**common), **args)
    for k, a, b in zip(res._fields, res, plain):
        assert torch.equal(a, b), k
    assert (res.status == 1).all()
    # what a Correlate records is what it was, and it has no structure factors
    tgo._same_accumulators(obs, obs_c)
    assert torch.equal(obs.vacf_sum, obs_c.vacf_sum) and torch.equal(obs.vacf_count, obs_c.vacf_count) and torch.equal(obs.frames_vel, obs_c.frames_vel)
    assert torch.equal(obs.frames_pos, obs_c.frames_pos)
    assert all(getattr(obs_c, k) is None for k in ("qvec", "sq_sum", "sq_frames", "sq_flag", "cell_sum", "fqt_sum", "fqt_count"))
    Q = len(QVEC)
    assert tuple(obs.sq_sum.shape) == (B, 6, Q) and tuple(obs.fqt_sum.shape) == (B, 6, 4, Q) and tuple(obs.fqt_count.shape) == (B, 4)
    assert (obs.sq_frames == STEPS - 1).all() and not obs.sq_flag.any()
    assert obs.fqt_count.cpu().tolist() == [[len([s for s in range(l, STEPS - 1) if (s - l) % 2 == 0]) for l in range(4)]] * B
    pbc, cell0 = _t(np.asarray(case.p["pbc"], np.int32)), _t(np.asarray(case.p["cell"], np.float64))
    want = torch.zeros_like(obs.cell_sum)
    for _ in range(STEPS - 1):                                   # the cell of every counted frame, added one by one
        want = want + cell0.view(B, 9)
    assert torch.equal(obs.cell_sum, want)
    _same_sq(obs, _replay(obs, types, node_ptr, request, STEPS, pbc, cell0))
    # S_aa at n = 0 is the number of atoms of the type, exactly
    totals = obs.type_totals.double()
    for a in range(3):
        s = obs.sq(a, a)[:, 0]
        has = totals[:, a] > 0
        assert torch.equal(s[has], totals[has, a]) and torch.isnan(s[~has]).all()
    # the helpers on the device tensors
    assert tuple(obs.q().shape) == (B, Q, 3) and tuple(obs.q_norm().shape) == (B, Q) and not obs.q_norm()[:, 0].any()
    assert tuple(obs.fqt(0, 1).shape) == (B, 4, Q) and tuple(obs.sq_radial(0, 0, 6.0, 12)[1].shape) == (B, 12)
    f0 = obs.fqt(0, 0)[:, 0]
    assert torch.isfinite(f0[totals[:, 0] > 0]).all()


def test_sample_with_a_scatter_under_npt_is_md_npt_to_the_bit():
    from matdeeplearn_amd import forces, ops
    case = trh.cgcnn_case()
    n = int(case.p["node_ptr"][1])
    model, masses, structs = tgm._oracle_model(), tmh.md_masses(case)[:n], case.structs[:1]
    fixed = np.zeros(n, bool)
    fixed[::5] = True
    npt = dict(pressure=3e-5, tau_p=1.0, compressibility=30.0, max_strain=0.03)
    args = dict(kT=2e-5, seed=11, fixed=fixed)
    types = tgo._types(case)[:n]
    common = dict(every=1, skip=2, rdf=tgo.RDF, msd=tgo.MSD, frames_every=1, types=types, vacf=tgv.VACF)
    request = forces.Scatter(sq=SQ, **common)
    with ops.deterministic():
        plain = forces.md_npt(model, structs, DIST_RANGE, masses, 1.0, STEPS, **npt, **args)
        res, obs = forces.sample(model, structs, DIST_RANGE, masses, 1.0, STEPS, request, npt=npt, **args)
        _, obs_c = forces.sample(model, structs, DIST_RANGE, masses, 1.0, STEPS, forces.Correlate(**common), npt=npt, **args)
    assert isinstance(res, forces.NPTResult)
    for k, a, b in zip(res._fields, res, plain):
        assert torch.equal(a, b), k
    assert (res.status == 1).all() and not torch.equal(obs.frames_cell[1], obs.frames_cell[0])          # the barostat acted
    tgo._same_accumulators(obs, obs_c)
    assert torch.equal(obs.vacf_sum, obs_c.vacf_sum) and torch.equal(obs.vacf_count, obs_c.vacf_count)
    pbc = _t(np.asarray(case.p["pbc"], np.int32)[:1])
    _same_sq(obs, _replay(obs, types, case.p["node_ptr"][:2], request, STEPS, pbc, None, obs.frames_cell))
    # the mean cell is that of the sampled frames, and S_aa at n = 0 is N_a whatever the cell does
    mean = obs.frames_cell[2:].sum(0).view(1, 9) / (STEPS - 1)
    assert torch.allclose(obs.cell_sum / obs.sq_frames.double().unsqueeze(1), mean, rtol=1e-14, atol=0)
    totals = obs.type_totals.double()
    for a in range(3):
        if totals[0, a] > 0:
            assert torch.equal(obs.sq(a, a)[:, 0], totals[:, a])


def test_sample_launches_the_scattering_kernels_once_per_sampled_step_and_never_otherwise():
    from matdeeplearn_amd import forces
    case = trh.cgcnn_case()
    model, masses = tgm._oracle_model(), tmh.md_masses(case)
    steps, every, skip, frames_every = 9, 3, 2, 4
    new = ("mdl_density_modes", "mdl_sq_accumulate")
    common = dict(every=every, skip=skip, rdf=tgo.RDF, msd=tgo.MSD, frames_every=frames_every, types=tgo._types(case), vacf=tgv.VACF)
    forces.md(model, case.structs, DIST_RANGE, masses, 1.0, 1, **tgo._run_args(case))     # (what a model asks the library once stays out of the lists)
    names = tgl.record(lambda: forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, steps, forces.Scatter(sq=SQ, **common), **tgo._run_args(case)))
    segments, current = [], []
    for name in names:                                          # what the loop called in front of every integrator launch
        current.append(name)
        if name == "mdl_md_step":
            segments.append(current)
            current = []
    assert len(segments) == steps + 1 and not set(new) & set(current)
    for it, seg in enumerate(segments):
        sampled = it >= skip and (it - skip) % every == 0
        assert seg.count(new[0]) == seg.count(new[1]) == (1 if sampled else 0), (it, seg)
        if sampled:                                             # behind the displacement launch, modes first
            i = seg.index("mdl_msd_accumulate")
            assert seg[i + 1:i + 3] == list(new), (it, seg)
    old = tgl.record(lambda: forces.sample(model, case.structs, DIST_RANGE, masses, 1.0, steps, forces.Correlate(**common), **tgo._run_args(case)))
    assert not set(new) & set(old) and old == [n for n in names if n not in new]
