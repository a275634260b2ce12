"""CPU checks of the time-correlation layer (forces.Correlate, ops.md_onstep_velocity, ops.vacf_accumulate; csrc/vacf.hip,
include/mdl_hip_dynamics.h), and the fp64 numpy restatements that tests/test_gpu_vacf.py compares the kernels with:

  onstep_velocity_reference   the velocity at the evaluated positions: the closing half kick as ONE correctly rounded multiply-add per
                              component (formed exactly in rationals and rounded once), so the kernel's bits can be asked for.
  vacf_reference              the correlation sums, structure by structure, and beside every accumulator word the sum of the
                              magnitudes of its terms: what a rounding bound is a multiple of.

The restatements are checked here against cases with known answers: ballistic motion, and harmonic wells driven through
test_md_host.md_reference, whose velocity-Verlet trajectory is known in closed form: x_n = x_eq + a cos(theta n) + b sin(theta n) with
cos(theta) = 1 - (omega dt)^2 / 2, and the on-step velocity (x_(n+1) - x_(n-1)) / (2 dt) = v_0 cos(theta n) - (a sin(theta) / dt)
sin(theta n) = A cos(theta n + phi)."""
import fractions
import inspect
import math
import os
import re

import numpy as np
import pytest
import torch

import test_md_host as tmh
import test_observe_host as toh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def fma(a, b, c):
    """a * b + c elementwise with ONE rounding (finite fp64 operands): exact in rationals, and float() of a rational rounds to
    nearest even"""
    a, b, c = np.broadcast_arrays(np.asarray(a, np.float64), np.asarray(b, np.float64), np.asarray(c, np.float64))
    F = fractions.Fraction
    out = np.array([float(F(float(x)) * F(float(y)) + F(float(z))) for x, y, z in zip(a.ravel(), b.ravel(), c.ravel())], np.float64)
    return out.reshape(a.shape)


def onstep_velocity_reference(vel, force, mass, fixed, node_ptr, dt, steps, status, out=None):
    """mdl_md_onstep_velocity in numpy: out [N, 3] (a copy of `out`, or zeros, with the rows of every running structure written).
    force is taken as it is: an fp32 array, which is what the kernel is handed, widens exactly."""
    vel, mass = np.asarray(vel, np.float64), np.asarray(mass, np.float64)
    force = np.asarray(force).astype(np.float64)
    out = np.zeros_like(vel) if out is None else np.array(out, np.float64)
    for b in range(len(node_ptr) - 1):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        if e == a or (status is not None and status[b] != 0):
            continue
        v = vel[a:e].copy()
        if steps[b] > 0:
            v = fma(0.5 * float(dt[b]), force[a:e] / mass[a:e, None], v)
        if fixed is not None:
            v[np.asarray(fixed[a:e]) != 0] = 0.0
        out[a:e] = v
    return out


def vacf_reference(v, origins, lag, mass, types, fixed, node_ptr, status, remove_com, T, n_lags, acc=None):
    """mdl_vacf_accumulate in numpy: (vacf_sum [B, 2, T, n_lags], vacf_count [B, n_lags], abs_sum [B, 2, T, n_lags] — the sum of the
    magnitudes of the terms of every word) after one frame.  acc: the three arrays to add to (copied), or None for zeros."""
    B = len(node_ptr) - 1
    vs, vc, va = ((np.zeros((B, 2, T, n_lags)), np.zeros((B, n_lags), np.int64), np.zeros((B, 2, T, n_lags))) if acc is None
                  else tuple(x.copy() for x in acc))
    for b in range(B):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        if e == a or (status is not None and status[b] != 0):
            continue
        free = np.ones(e - a, bool) if fixed is None else np.asarray(fixed[a:e]) == 0
        m, t = np.asarray(mass[a:e], np.float64)[free], np.asarray(types[a:e])[free]
        for k, lg in enumerate(lag):
            if lg < 0 or lg >= n_lags:
                continue
            u, u0 = np.asarray(v[a:e], np.float64)[free], np.asarray(origins[k, a:e], np.float64)[free]
            if remove_com and m.sum() > 0:
                u, u0 = u - (m[:, None] * u).sum(0) / m.sum(), u0 - (m[:, None] * u0).sum(0) / m.sum()
            d = (u * u0).sum(1)
            for ty in range(T):
                sel = t == ty
                vs[b, 0, ty, lg] += d[sel].sum()
                vs[b, 1, ty, lg] += (m[sel] * d[sel]).sum()
                va[b, 0, ty, lg] += np.abs(d[sel]).sum()
                va[b, 1, ty, lg] += (m[sel] * np.abs(d[sel])).sum()
            vc[b, lg] += 1
    return vs, vc, va


def observations(vacf_sum, vacf_count, type_counts, lag_time):
    """a forces.Observations around host arrays: its helpers are torch arithmetic and run anywhere"""
    from matdeeplearn_amd import forces
    o = forces.Observations.__new__(forces.Observations)
    o.vacf_sum, o.vacf_count = torch.from_numpy(np.asarray(vacf_sum, np.float64)), torch.from_numpy(np.asarray(vacf_count, np.int64))
    o.type_counts, o.lag_time = torch.from_numpy(np.asarray(type_counts, np.int64)), torch.from_numpy(np.asarray(lag_time, np.float64))
    return o


# ---------------------------------------------------------------------------------------------
# 1. the surface
# ---------------------------------------------------------------------------------------------
def test_dynamics_header_and_prototype_table_agree_and_the_other_two_layers_are_what_they_were():
    from matdeeplearn_amd import _build, _lib, ops
    header = open(os.path.join(ROOT, "include", "mdl_hip_dynamics.h")).read()
    declared = toh._declared("mdl_hip_dynamics.h")
    assert declared == set(_lib.DYNAMICS_PROTOTYPES) == {"mdl_md_onstep_velocity", "mdl_vacf_accumulate"}
    assert not declared & set(_lib.PROTOTYPES) and not declared & set(_lib.ANALYSIS_PROTOTYPES)
    assert set(_lib.ANALYSIS_PROTOTYPES) == toh._declared("mdl_hip_analysis.h") == {"mdl_rdf_accumulate", "mdl_msd_accumulate"}
    assert len(toh._declared("mdl_hip.h")) == 84 == len(_lib.PROTOTYPES) and len(_lib.PROTOTYPES["mdl_md_step"][1]) == 25
    for name, (res, args) in _lib.DYNAMICS_PROTOTYPES.items():
        proto = re.search(r"\b%s\s*\(([^)]*)\)" % name, header).group(1)
        assert len(proto.split(",")) == len(args), name
    assert len(_lib.DYNAMICS_PROTOTYPES["mdl_md_onstep_velocity"][1]) == 12 and len(_lib.DYNAMICS_PROTOTYPES["mdl_vacf_accumulate"][1]) == 17
    if os.path.exists(_build.LIB):
        handle = _lib.lib()
        for name in declared:
            assert hasattr(handle, name), name
            assert getattr(handle, name).argtypes == _lib.DYNAMICS_PROTOTYPES[name][1]
    assert _build.FILE_FLAGS["vacf.hip"] == ["-ffp-contract=off"]
    assert ops.VacfState.__slots__ == ("types", "node_ptr", "n_types", "n_lags", "origins", "vacf_sum", "vacf_count")
    assert "vacf" not in " ".join(ops.ObserveState.__slots__)


def test_correlate_is_an_observe_and_the_pinned_signatures_stand():
    from matdeeplearn_amd import forces, ops
    assert issubclass(forces.Correlate, forces.Observe)
    assert str(inspect.signature(forces.Correlate)) == "(every=1, skip=0, rdf=None, msd=None, frames_every=0, types=None, vacf=None)"
    assert str(inspect.signature(forces.sample)) == "(model, structs, dist_range, masses, dt, steps, observe, npt=None, **md_kwargs)"
    assert str(inspect.signature(forces.Observe)) == "(every=1, skip=0, rdf=None, msd=None, frames_every=0, types=None)"
    assert str(inspect.signature(ops.md_onstep_velocity)) == "(vel, force, mass, node_ptr, state, dt, fixed=None, out=None)"
    assert str(inspect.signature(ops.vacf_state)) == "(types, node_ptr, n_types=None, vacf=None, device=None)"
    assert str(inspect.signature(ops.vacf_accumulate)) == "(v, lag, mass, state, fixed=None, status=None, remove_com=True)"
    c = forces.Correlate()
    assert (c.every, c.skip, c.rdf, c.msd, c.frames_every, c.types, c.vacf) == (1, 0, None, None, 0, None, None)
    c = forces.Correlate(every=2, msd=dict(n_lags=8, origin_every=2), vacf=dict(n_lags=64, origin_every=4))
    assert c.vacf == dict(n_lags=64, origin_every=4, n_origins=16, remove_com=True) and c.msd["n_origins"] == 4 and c.every == 2
    assert forces.Correlate(vacf=dict(n_lags=5, origin_every=2, remove_com=False, n_origins=7)).vacf == dict(n_lags=5, origin_every=2, n_origins=7,
                                                                                                             remove_com=False)
    for k in ("vacf_sum", "vacf_count", "frames_vel", "vacf", "vdos", "diffusion_gk"):
        assert k in inspect.getsource(forces.Observations), k
    # only a Correlate that has something to ask of the velocities gets _md's second hook
    from matdeeplearn_amd.process import graph as pg
    p = pg.pack_structures(toh._structs())
    hook = lambda req: forces._Observer(req, p, 6).velocities
    assert not hook(forces.Observe(frames_every=1)) and not hook(forces.Correlate(msd=dict(n_lags=2)))
    assert hook(forces.Correlate(frames_every=3)) and hook(forces.Correlate(vacf=dict(n_lags=2)))


def test_argument_errors_raise_before_a_device_is_needed():
    from matdeeplearn_amd import forces, ops
    E = ops.MdlError
    for vacf, msg in ((dict(n_lags=0), "vacf: n_lags must be >= 1"), (dict(n_lags=4, origin_every=0), "vacf: origin_every must be >= 1"),
                      (dict(origin_every=2), "vacf must be dict"), (dict(n_lags=4, every=2), "vacf must be dict"),
                      (dict(n_lags=4, n_origins=0), "vacf: n_origins must be in 1"), (dict(n_lags=4, n_origins=65536), "vacf: n_origins must be in 1")):
        with pytest.raises(E, match=msg):
            forces.Correlate(vacf=vacf)
        with pytest.raises(E, match=msg):
            ops.vacf_state([0, 0, 1], [0, 3], vacf=vacf, device="cpu")
    with pytest.raises(E, match="every must be >= 1"):
        forces.Correlate(every=0, vacf=dict(n_lags=2))
    # what needs the structures: forces.sample raises before it looks at the model (None here) or at a device
    structs, masses = toh._structs(), np.ones(5)
    run = lambda o, **kw: forces.sample(None, structs, (0.0, 8.0), masses, 1.0, 4, o, **kw)
    with pytest.raises(E, match="vacf: at most 64 types"):
        run(forces.Correlate(vacf=dict(n_lags=4), types=[0, 1, 2, 3, 70]))
    with pytest.raises(E, match=r"Observe.types must be \[N\] with N = 5"):
        run(forces.Correlate(vacf=dict(n_lags=4), types=[0, 1]))
    with pytest.raises(E, match="energy_and_forces"):                            # past the observer's checks: the model is looked at
        run(forces.Correlate(vacf=dict(n_lags=4)))
    # ops.vacf_state
    with pytest.raises(E, match="vacf must be dict"):
        ops.vacf_state([0, 1], [0, 2], device="cpu")
    with pytest.raises(E, match=r"types must be in 0 \.\. 1"):
        ops.vacf_state([0, 1, 2], [0, 3], n_types=2, vacf=dict(n_lags=2), device="cpu")
    with pytest.raises(E, match="node_ptr must start at 0"):
        ops.vacf_state([0, 1, 2, 3], [0, 3], vacf=dict(n_lags=2), device="cpu")
    with pytest.raises(E, match="at most 64 types"):
        ops.vacf_state([0, 64], [0, 2], vacf=dict(n_lags=2), device="cpu")
    with pytest.raises(E, match="integer"):
        ops.vacf_state([0.5, 1.0], [0, 2], vacf=dict(n_lags=2), device="cpu")
    st = ops.vacf_state([0, 1, 2, 3], [0, 1, 4], vacf=dict(n_lags=3, origin_every=2), device="cpu")
    assert (st.n_types, st.n_lags, tuple(st.origins.shape), tuple(st.vacf_sum.shape), tuple(st.vacf_count.shape)) == (4, 3, (2, 4, 3), (2, 2, 4, 3), (2, 3))
    assert st.types.dtype == torch.int32 and st.node_ptr.dtype == torch.int64 and st.vacf_count.dtype == torch.int64 and not st.vacf_sum.any()
    # ops.vacf_accumulate
    v, mass, lag = torch.zeros(4, 3, dtype=torch.float64), torch.ones(4, dtype=torch.float64), torch.zeros(2, dtype=torch.int32)
    acc = lambda **kw: ops.vacf_accumulate(*[dict(dict(v=v, lag=lag, mass=mass, state=st, fixed=None, status=None), **kw)[k]
                                             for k in ("v", "lag", "mass", "state", "fixed", "status")])
    for kw, msg in ((dict(v=v.float()), "v must be a contiguous"), (dict(v=v[:3]), "v must be"), (dict(v=v.t().contiguous().t()), "v must be a contiguous"),
                    (dict(lag=lag[:1]), "lag must be"), (dict(lag=lag.long()), "lag must be"), (dict(mass=mass.float()), "mass must be"),
                    (dict(mass=mass[:3]), "mass must be"), (dict(fixed=torch.zeros(4, dtype=torch.int32)), "fixed must be"),
                    (dict(status=torch.zeros(2, dtype=torch.int64)), "status must be"), (dict(status=torch.zeros(3, dtype=torch.int32)), "status must be"),
                    (dict(state=None), "state must be an ops.VacfState"),
                    (dict(state=ops.observe_state([0, 1, 2, 3], [0, 1, 4], msd=dict(n_lags=3), device="cpu")), "state must be an ops.VacfState"),
                    (dict(), "HIP device")):
        with pytest.raises(E, match=msg):
            acc(**kw)
    # ops.md_onstep_velocity
    state, node_ptr, force = ops.md_state(2, "cpu"), torch.tensor([0, 1, 4]), torch.zeros(4, 3)
    ons = lambda **kw: ops.md_onstep_velocity(*[dict(dict(vel=v, force=force, mass=mass, node_ptr=node_ptr, state=state, dt=0.5, fixed=None, out=None), **kw)[k]
                                                for k in ("vel", "force", "mass", "node_ptr", "state", "dt", "fixed", "out")])
    for kw, msg in ((dict(state=None), "state must be an ops.MDState"), (dict(state=st), "state must be an ops.MDState"),
                    (dict(vel=v.float()), "vel must be a contiguous"), (dict(force=force.double()), "force must be"), (dict(force=force[:3]), "force must be"),
                    (dict(mass=mass[:3]), "mass must be"), (dict(node_ptr=node_ptr.int()), "node_ptr must be"),
                    (dict(node_ptr=torch.tensor([0, 1, 2, 4])), r"state.steps must be a contiguous \[3\]"), (dict(dt=0.0), "dt must be > 0"),
                    (dict(dt=float("nan")), "dt must be > 0"), (dict(dt=torch.ones(3, dtype=torch.float64)), "dt must be a number or"),
                    (dict(dt=torch.ones(2)), "dt must be a number or"), (dict(fixed=torch.zeros(3, dtype=torch.uint8)), "fixed must be"),
                    (dict(out=torch.zeros(4, 3)), "out must be"), (dict(out=torch.zeros(3, 3, dtype=torch.float64)), "out must be"),
                    (dict(), "HIP device"), (dict(state=ops.md_cell_state(2, "cpu")), "HIP device")):
        with pytest.raises(E, match=msg):
            ons(**kw)
    # the helpers say what they were not asked for, and what they need
    o = observations(np.zeros((1, 2, 1, 1)), np.ones((1, 1)), [[1]], [1.0])
    with pytest.raises(E, match="n_lags >= 2"):
        o.vdos(0)
    with pytest.raises(E, match="lag_hi"):
        o.diffusion_gk(0, 2)
    o.vacf_sum = None
    for call in (lambda: o.vacf(0), lambda: o.vdos(0), lambda: o.diffusion_gk(0, 1)):
        with pytest.raises(E, match="not asked for it"):
            call()


# ---------------------------------------------------------------------------------------------
# 2. the references against cases with known answers
# ---------------------------------------------------------------------------------------------
def test_the_rational_multiply_add_rounds_once():
    # 1 + 2^-53 is a tie that a separate product and sum round away; the fused result keeps the low bit of the exact value
    a, b, c = 1.0 + 2.0 ** -52, 1.0 - 2.0 ** -53, -1.0
    assert a * b + c != fma(a, b, c) and float(fma(a, b, c)) == 2.0 ** -53 - 2.0 ** -105
    rng = np.random.default_rng(0)
    x, y, z = rng.normal(size=(3, 200))
    assert np.abs(fma(x, y, z) - (x * y + z)).max() <= 2.0 ** -52 * np.abs(x * y + z).max() and fma(x, y, z).shape == (200,)


def test_ballistic_motion_has_a_flat_vacf_and_a_linear_green_kubo_integral():
    from matdeeplearn_amd import ops
    rng = np.random.default_rng(5)
    node_ptr, T, n, n_lags, n_samples, dt = np.array([0, 4, 9]), 2, 9, 5, 12, 0.5
    types, mass = np.array([0, 1, 0, 1, 1, 0, 0, 1, 0]), rng.uniform(1, 3, 9)
    v = rng.normal(size=(2, 3))[types]                          # one velocity per type, constant in time
    slot, lag = ops.msd_schedule(n_samples, n_lags, 2, 3)
    origins, acc = np.zeros((3, n, 3)), None
    for s in range(n_samples):
        if slot[s] >= 0:
            origins[int(slot[s])] = v
        acc = vacf_reference(v, origins, lag[s].tolist(), mass, types, None, node_ptr, None, False, T, n_lags, acc)
    vs, vc, va = acc
    assert (vc > 0).all() and np.array_equal(vc[0], vc[1]) and np.allclose(vs, va, rtol=1e-15, atol=0)      # every term is |v|^2 > 0
    counts = np.array([[(types[node_ptr[b]:node_ptr[b + 1]] == t).sum() for t in range(T)] for b in range(2)])
    o = observations(vs, vc, counts, [dt, dt])
    for t in range(T):
        v2 = (v[types == t][0] ** 2).sum()
        assert np.allclose(o.vacf(t).numpy(), v2, rtol=1e-13, atol=0)
        for b in range(2):
            m = mass[node_ptr[b]:node_ptr[b + 1]][types[node_ptr[b]:node_ptr[b + 1]] == t]
            assert np.allclose(o.vacf(t, mass_weighted=True)[b].numpy(), v2 * m.mean(), rtol=1e-13, atol=0)
        for hi in range(1, n_lags + 1):                        # the integral of a constant over (hi - 1) intervals
            assert np.allclose(o.diffusion_gk(t, hi).numpy(), v2 * (hi - 1) * dt / 3.0, rtol=1e-13, atol=0)
    # equal velocities are the centre of mass: nothing is left once it is removed
    same = np.tile(v[:1], (n, 1))
    vs0, vc0, _ = vacf_reference(same, same[None], [0], mass, types, None, node_ptr, None, True, T, 1)
    assert (vc0 == 1).all() and np.abs(vs0).max() <= 1e-28 * (same ** 2).sum()
    # a type nobody has and a lag nobody reached are NaN
    o = observations(np.zeros((1, 2, 2, 3)), [[2, 1, 0]], [[3, 0]], [dt])
    assert np.isnan(o.vacf(1).numpy()).all() and np.isnan(o.vacf(0).numpy()).tolist() == [[False, False, True]]
    assert np.isnan(o.vdos(0)[1].numpy()).all()


PERIOD = 16                                                     # samples per oscillation
OMEGA_DT = math.sqrt(2.0 * (1.0 - math.cos(2.0 * math.pi / PERIOD)))      # cos(theta) = 1 - (omega dt)^2 / 2 with theta = 2 pi / PERIOD


def _wells_run(n_steps, sizes=(5, 1, 9), seed=3):
    """NVE in harmonic wells through tmh.md_reference: per evaluation the raw vel, the on-step velocity of the reference above and
    the integrator's ekin; and the closed form's (A, phi) of every velocity component"""
    node_ptr, dt, mass, k, x0, rng = tmh._wells(seed, list(sizes), OMEGA_DT)
    pos = x0 + 0.1 * rng.normal(size=x0.shape)
    vel = 0.3 * rng.normal(size=x0.shape)
    dt_atom = np.repeat(dt, sizes)[:, None]
    theta = 2.0 * math.pi / PERIOD
    amp_sin = (pos - x0) * math.sin(theta) / dt_atom            # v_n = v_0 cos(theta n) - amp_sin sin(theta n)
    A, phi = np.sqrt(vel ** 2 + amp_sin ** 2), np.arctan2(amp_sin, vel)
    st = tmh.new_state(len(sizes))
    raw, onstep, ekin = [], [], []
    for _ in range(n_steps + 1):
        f = -k * (pos - x0)
        raw.append(vel.copy())
        onstep.append(onstep_velocity_reference(vel, f, mass, None, node_ptr, dt, st["steps"], st["status"]))
        pos, vel, st, _ = tmh.md_reference(pos, vel, f, mass, node_ptr, st, dt, n_steps)
        ekin.append(st["ekin"].copy())
    assert (st["status"] == 1).all()
    return node_ptr, dt, mass, np.array(raw), np.array(onstep), np.array(ekin), A, phi


def test_the_on_step_velocity_has_the_integrators_kinetic_energy_and_the_stored_velocity_has_not():
    """what separates the on-step velocity from `vel`: half the mass-weighted lag-0 sum (remove_com off) IS the integrator's ekin"""
    n_steps = 40
    node_ptr, dt, mass, raw, onstep, ekin, _, _ = _wells_run(n_steps)
    N, B = len(mass), len(node_ptr) - 1
    types = np.arange(N) % 3
    worst_on, least_raw = 0.0, math.inf
    for it in range(n_steps + 1):
        for v, is_onstep in ((onstep[it], True), (raw[it], False)):
            vs, vc, _ = vacf_reference(v, v[None], [0], mass, types, None, node_ptr, None, False, 3, 1)
            half = 0.5 * vs[:, 1, :, 0].sum(1)
            rel = np.abs(half - ekin[it]) / ekin[it]
            if is_onstep:
                worst_on = max(worst_on, rel.max())
                assert (rel <= 1e-12).all(), (it, rel)
            elif it > 0:                                        # (at the first evaluation vel IS the on-step velocity)
                least_raw = min(least_raw, rel.min())
                assert (rel > 1e-6).all(), (it, rel)
    assert np.array_equal(onstep[0], raw[0])
    print("on-step: within %.1e of ekin (bound 1e-12); vel: at least %.1e away (bound 1e-6)" % (worst_on, least_raw))


@pytest.mark.parametrize("origin_every", [1, 3])
def test_harmonic_wells_have_the_closed_form_vacf_and_a_vdos_peak_at_their_frequency(origin_every):
    from matdeeplearn_amd import ops
    n_lags, n_steps = 2 * PERIOD + 1, 5 * PERIOD
    node_ptr, dt, mass, raw, onstep, ekin, A, phi = _wells_run(n_steps)
    N, B, T = len(mass), len(node_ptr) - 1, 2
    types = np.arange(N) % T
    n_samples = n_steps + 1
    K = -(-n_lags // origin_every)
    slot, lag = ops.msd_schedule(n_samples, n_lags, origin_every, K)
    origins, acc = np.zeros((K, N, 3)), None
    for s in range(n_samples):
        if slot[s] >= 0:
            origins[int(slot[s])] = onstep[s]
        acc = vacf_reference(onstep[s], origins, lag[s].tolist(), mass, types, None, node_ptr, None, False, T, n_lags, acc)
    vs, vc, _ = acc
    theta = 2.0 * math.pi / PERIOD
    want = np.zeros_like(vs)
    worst = 0.0
    for b in range(B):
        sl = slice(node_ptr[b], node_ptr[b + 1])
        for n in range(n_lags):
            s0 = np.arange(0, n_samples - n, origin_every)      # the origins whose lag n was sampled
            assert vc[b, n] == len(s0) > 0
            ph = phi[sl][None] + theta * s0[:, None, None]      # [origins, atoms, 3]
            terms = (A[sl][None] ** 2 * np.cos(ph) * np.cos(ph + theta * n)).sum((0, 2))
            for t in range(T):
                sel = types[sl] == t
                want[b, 0, t, n], want[b, 1, t, n] = terms[sel].sum(), (mass[sl][sel] * terms[sel]).sum()
        scale = (A[sl] ** 2).max()
        for plane, m_scale in ((0, 1.0), (1, mass[sl].max())):
            err = np.abs(vs[b, plane] - want[b, plane]).max() / (scale * m_scale)
            worst = max(worst, err)
            assert err <= 1e-9, (b, plane, err)
    print("the reference VACF is within %.1e A^2 of the closed form (bound 1e-9)" % worst)
    # the spectrum: one line at Omega / 2 pi = 1 / (PERIOD dt), the bin 2 M / PERIOD of freq_k = k / (2 M dt)
    counts = np.array([[(types[node_ptr[b]:node_ptr[b + 1]] == t).sum() for t in range(T)] for b in range(B)])
    o = observations(vs, vc, counts, dt)
    M = n_lags - 1
    for t in range(T):
        for window in (True, False):
            freq, dos = o.vdos(t, window=window)
            freq, dos = freq.numpy(), dos.numpy()
            for b in range(B):
                if counts[b, t] == 0:
                    assert np.isnan(dos[b]).all()
                    continue
                peak = int(np.argmax(dos[b]))
                assert peak == 2 * M // PERIOD == int(np.argmin(np.abs(freq[b] - 1.0 / (PERIOD * dt[b])))), (b, t, window, peak)
                assert np.allclose(freq[b], np.arange(n_lags) / (2.0 * M * dt[b]), rtol=1e-15, atol=0)


def test_the_density_of_states_integrates_to_the_degrees_of_freedom():
    """sum''_k dos_k / (2 M dt) = 3 N_t: the inverse DCT-I at n = 0, for any correlation function"""
    rng = np.random.default_rng(11)
    B, T = 3, 2
    for n_lags in (2, 3, 17, 64):
        vs = rng.normal(size=(B, 2, T, n_lags))
        vs[:, :, :, 0] = np.abs(vs[:, :, :, 0]) + 1.0
        counts, dt = rng.integers(1, 9, (B, T)), rng.uniform(0.1, 2.0, B)
        o = observations(vs, rng.integers(1, 5, (B, n_lags)), counts, dt)
        M = n_lags - 1
        for t in range(T):
            for window in (True, False):
                dos = o.vdos(t, window=window)[1].numpy()
                total = (dos.sum(1) - 0.5 * (dos[:, 0] + dos[:, M])) / (2.0 * M * dt)
                assert (np.abs(total - 3.0 * counts[:, t]) <= 1e-10 * 3.0 * counts[:, t]).all(), (n_lags, t, window, total)
