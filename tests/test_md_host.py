"""Host side of the molecular-dynamics tests: this file OWNS the fp64 numpy restatements of csrc/md.hip as include/mdl_hip.h states
it — philox4x32_10, md_noise_reference, md_reference (ops.md_step) and md_velocities_reference (ops.md_velocities) — and the fp64
reference trajectory of the oracle CGCNN at held neighbour lists that tests/test_gpu_md.py compares forces.md with.  The upstream
reference moves no atoms, so no golden from it exists.  No GPU.

MD_TRAJ_BOUND, the bound of that comparison, is the reference's own sensitivity (the recipe of test_relax_host.TRAJ_BOUND): the same
50 NVE steps with every force perturbed by uniform noise of amplitude 1e-4 max|F| moved the final positions by DEV = 3.12e-5 A at
most (measured here; the atoms travel up to 1.03 A); MD_TRAJ_BOUND = 10 x DEV, rounded up to two digits.  MD_ENERGY_EXCURSION is the
largest |E(n) - E(0)| of prediction + kinetic energy along that fp64 trajectory, per structure (measured here, rounded up to two
digits): the integrator's own O(dt^2) oscillation, which the device run may not exceed by more than a factor of two."""
import functools

import numpy as np
import pytest
import torch

import test_relax_host as trh

MD_TRAJ_BOUND = 3.2e-4        # A; 10 x the DEV measured below (see the module docstring)
MD_ENERGY_EXCURSION = np.array([3.9e-7, 1.7e-6, 5.2e-7, 3.8e-7, 3.3e-6, 6.0e-6])     # per structure of trh.cgcnn_case(), measured below
MD_ARGS = dict(steps=50, dt=1.0)
MD_KT_INIT, MD_SEED = 2e-5, 7


# ---------------------------------------------------------------------------------------------
# the restatements
# ---------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """Philox4x32-10 (Salmon et al., SC'11): counter [..., 4], key [..., 2] (anything that broadcasts) uint32 -> [..., 4] uint32"""
    c = [np.asarray(counter, dtype=np.uint64)[..., k] & np.uint64(0xFFFFFFFF) for k in range(4)]
    k0, k1 = [np.asarray(key, dtype=np.uint64)[..., k] & np.uint64(0xFFFFFFFF) for k in range(2)]
    mask, m0, m1 = np.uint64(0xFFFFFFFF), np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
    for _ in range(10):
        p0, p1 = m0 * c[0], m1 * c[2]                          # 32 x 32 -> 64 bits: no overflow in uint64
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k0, p1 & mask, (p0 >> np.uint64(32)) ^ c[3] ^ k1, p0 & mask]
        k0, k1 = (k0 + np.uint64(0x9E3779B9)) & mask, (k1 + np.uint64(0xBB67AE85)) & mask
    return np.stack(np.broadcast_arrays(*c), -1).astype(np.uint32)


def md_noise_reference(n_atoms, step, tag, seed):
    """[n_atoms, 3] standard normal numbers of one structure: counter (atom, 0, step, tag), key (low, high) half of seed"""
    s = int(seed) & 0xFFFFFFFFFFFFFFFF
    ctr = np.zeros((int(n_atoms), 4), np.uint64)
    ctr[:, 0], ctr[:, 2], ctr[:, 3] = np.arange(int(n_atoms)), int(step), int(tag)
    w = philox4x32_10(ctr, np.array([s & 0xFFFFFFFF, s >> 32], np.uint64)).astype(np.float64)
    u = (w + 0.5) * 2.0 ** -32
    r0, r1 = np.sqrt(-2.0 * np.log(u[:, 0])), np.sqrt(-2.0 * np.log(u[:, 2]))
    return np.stack([r0 * np.cos(2.0 * np.pi * u[:, 1]), r0 * np.sin(2.0 * np.pi * u[:, 1]), r1 * np.cos(2.0 * np.pi * u[:, 3])], 1)


def new_state(B):
    return {"steps": np.zeros(B, np.int32), "status": np.zeros(B, np.int32), "ekin": np.zeros(B)}


def _per_structure(v, B, dtype):
    return np.broadcast_to(np.asarray(v, dtype=dtype), (B,))


def _seeds(seed, B):
    return np.asarray(seed, np.int64) if np.ndim(seed) else int(seed) + np.arange(B, dtype=np.int64)


def md_reference(pos, vel, force, mass, node_ptr, state, dt, n_steps, gamma=0.0, kT=0.0, seed=0, fixed=None, max_disp=0.5):
    """One call of ops.md_step for every structure, fp64, one structure after the other.  Returns (pos, vel, state, diag) as NEW
    arrays; diag[b]: the branch structure b took and the displacements |x'' - x| of its free atoms its guard decided on."""
    pos, vel = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
    force, mass = np.asarray(force, dtype=np.float64), np.asarray(mass, dtype=np.float64)
    st = {k: np.array(v) for k, v in state.items()}
    B = len(node_ptr) - 1
    dt, gamma, kT = [_per_structure(v, B, np.float64) for v in (dt, gamma, kT)]
    n_steps, seed = _per_structure(n_steps, B, np.int32), _seeds(seed, B)
    free_all = np.ones(len(pos), bool) if fixed is None else ~np.asarray(fixed).astype(bool)
    diag = []
    for b in range(B):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        d = {"branch": "stopped", "disp": np.zeros(0)}
        diag.append(d)
        if st["status"][b] != 0:
            continue
        free = free_all[a:e][:, None]
        m, f, x, h, steps = mass[a:e][:, None], force[a:e], pos[a:e], 0.5 * dt[b], int(st["steps"][b])
        with np.errstate(all="ignore"):
            v = np.where(free, vel[a:e], 0.0)
            if steps > 0:
                v = np.where(free, v + h * (f / m), 0.0)
            st["ekin"][b] = 0.5 * np.where(free, m * v * v, 0.0).sum()
            if steps == n_steps[b]:
                vel[a:e], st["status"][b], d["branch"] = v, 1, "closing"
                continue
            v1 = v + h * (f / m)
            x1 = x + h * v1
            v2 = v1
            if gamma[b] > 0.0:
                c1, c2 = np.exp(-gamma[b] * dt[b]), np.sqrt(-np.expm1(-2.0 * gamma[b] * dt[b]))
                v2 = c1 * v1 + c2 * np.sqrt(kT[b] / m) * md_noise_reference(e - a, steps, 0, seed[b])
            x2 = x1 + h * v2
            d["disp"] = np.sqrt(((x2 - x) ** 2).sum(1))[free[:, 0]]
            if (~(d["disp"] <= max_disp)).sum() > 0:
                vel[a:e], st["status"][b], d["branch"] = v, 2, "refused"
                continue
        pos[a:e], vel[a:e] = np.where(free, x2, x), np.where(free, v2, 0.0)
        st["steps"][b] += 1
        d["branch"] = "langevin" if gamma[b] > 0.0 else "nve"
    return pos, vel, st, diag


def md_velocities_reference(mass, node_ptr, kT, seed=0, fixed=None, zero_momentum=True):
    """ops.md_velocities, fp64: [N, 3]"""
    mass = np.asarray(mass, dtype=np.float64)
    B = len(node_ptr) - 1
    kT, seed = _per_structure(kT, B, np.float64), _seeds(seed, B)
    free_all = np.ones(len(mass), bool) if fixed is None else ~np.asarray(fixed).astype(bool)
    vel = np.zeros((len(mass), 3))
    for b in range(B):
        a, e = int(node_ptr[b]), int(node_ptr[b + 1])
        free, m = free_all[a:e], mass[a:e][:, None]
        v = np.where(free[:, None], np.sqrt(kT[b] / m) * md_noise_reference(e - a, 0, 1, seed[b]), 0.0)
        if zero_momentum and free.sum() >= 2:
            v = np.where(free[:, None], v - (m * v)[free].sum(0) / m[free].sum(), 0.0)
        vel[a:e] = v
    return vel


# ---------------------------------------------------------------------------------------------
# 1. / 2. the noise
# ---------------------------------------------------------------------------------------------
def test_philox_known_answers():
    word = lambda s: [int(w, 16) for w in s.split()]
    for ctr, key, out in (("0 0 0 0", "0 0", "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
                          ("ffffffff ffffffff ffffffff ffffffff", "ffffffff ffffffff", "408f276d 41c83b0e a20bc7c6 6d5451fd"),
                          ("243f6a88 85a308d3 13198a2e 03707344", "a4093822 299f31d0", "d16cfe09 94fdcceb 5001e420 24126ea1")):
        got = philox4x32_10(np.array(word(ctr), np.uint32), np.array(word(key), np.uint32))
        assert [int(w) for w in got] == word(out), (ctr, key, ["%08x" % w for w in got])
    # vectorised over counters and keys alike
    both = philox4x32_10(np.array([word("0 0 0 0"), word("243f6a88 85a308d3 13198a2e 03707344")], np.uint32),
                         np.array([word("0 0"), word("a4093822 299f31d0")], np.uint32))
    assert [int(w) for w in both[0]] == word("6627e8d5 e169c58d bc57ac4c 9b00dbd8") and int(both[1, 3]) == 0x24126ea1


def test_noise_is_standard_normal_and_uncorrelated():
    """3 x 65536 values of one structure at (step 3, tag 0, seed 12345) and of another at (step 0, tag 1, a seed with a high half)"""
    n = 65536
    for step, tag, seed in ((3, 0, 12345), (0, 1, -(5 << 32) + 17)):
        xi = md_noise_reference(n, step, tag, seed)
        assert xi.shape == (n, 3) and np.isfinite(xi).all()
        mean, var = xi.mean(), xi.var()
        corr = [float((xi[:, i] * xi[:, j]).mean()) for i, j in ((0, 1), (0, 2), (1, 2))]
        print("mean %.3e (bound %.3e)  var - 1 %.3e (bound %.3e)  correlations %s (bound %.3e)"
              % (mean, 5 / np.sqrt(3 * n), var - 1, 5 * np.sqrt(2 / (3 * n)), corr, 5 / np.sqrt(n)))
        assert abs(mean) <= 5 / np.sqrt(3 * n)
        assert abs(var - 1.0) <= 5 * np.sqrt(2.0 / (3 * n))
        assert max(abs(c) for c in corr) <= 5 / np.sqrt(n)
    # the counter: another step, another tag or another key is another stream; the same is the same
    base = md_noise_reference(8, 3, 0, 12345)
    assert np.array_equal(base, md_noise_reference(8, 3, 0, 12345))
    assert all(not np.array_equal(base, md_noise_reference(8, *o)) for o in ((4, 0, 12345), (3, 1, 12345), (3, 0, 12346), (3, 0, 12345 + (1 << 32))))
    assert np.array_equal(base[:5], md_noise_reference(5, 3, 0, 12345))                   # an atom's numbers do not depend on the others


# ---------------------------------------------------------------------------------------------
# 3. NVE on harmonic wells
# ---------------------------------------------------------------------------------------------
def _wells(seed, sizes, omega_dt):
    """atoms in harmonic wells of their own: stiffness k_i, mass m_i, one dt per structure with omega_i dt = omega_dt"""
    rng = np.random.default_rng(seed)
    node_ptr = np.concatenate([[0], np.cumsum(sizes)])
    N, B = int(node_ptr[-1]), len(sizes)
    dt = rng.uniform(0.05, 0.2, B)
    mass = rng.uniform(1.0, 20.0, N)
    k = mass * (omega_dt / np.repeat(dt, sizes)) ** 2
    x0 = rng.uniform(0.0, 10.0, (N, 3))
    return node_ptr, dt, mass, k[:, None], x0, rng


def _run(pos, vel, force_of, mass, node_ptr, n, dt, record=None, **kw):
    """n steps: n + 1 calls of md_reference, each behind an evaluation of force_of"""
    st = new_state(len(node_ptr) - 1)
    for _ in range(n + 1):
        f = force_of(pos)
        new_pos, vel, st, _ = md_reference(pos, vel, f, mass, node_ptr, st, dt, n, **kw)
        if record is not None:
            record(pos, st)                                      # ekin belongs to the positions the forces were evaluated at
        pos = new_pos
    assert (st["status"] == 1).all() and (st["steps"] == n).all()
    return pos, vel, st


def test_nve_is_time_reversible_and_conserves_the_shadow_energy_of_harmonic_wells():
    node_ptr, dt, mass, k, x0, rng = _wells(3, [5, 1, 9], 0.1)
    pos0 = x0 + 0.1 * rng.normal(size=x0.shape)
    vel0 = 0.05 * rng.normal(size=x0.shape)
    force_of = lambda p: -k * (p - x0)                          # fp64: the rounding of fp32 forces is not reversible
    n = 200
    pos1, vel1, _ = _run(pos0, vel0, force_of, mass, node_ptr, n, dt)
    assert np.abs(pos1 - pos0).max() > 0.01
    pos2, vel2, _ = _run(pos1, -vel1, force_of, mass, node_ptr, n, dt)
    print("after n steps, v -> -v, n steps: |x - x0| %.3e  |v + v0| %.3e" % (np.abs(pos2 - pos0).max(), np.abs(vel2 + vel0).max()))
    assert np.abs(pos2 - pos0).max() <= 1e-10 and np.abs(vel2 + vel0).max() <= 1e-10
    # 1000 steps: E = sum 1/2 k x^2 + ekin oscillates; velocity Verlet conserves 1/2 m v^2 + 1/2 k x^2 (1 - (omega dt)^2 / 4) exactly
    total, shadow = [], []
    seg = lambda a: np.add.reduceat(a.sum(1), node_ptr[:-1])

    def record(p, st):
        pot = seg(0.5 * k * (p - x0) ** 2)
        total.append(pot + st["ekin"])
        shadow.append(pot * (1.0 - 0.1 ** 2 / 4) + st["ekin"])

    _run(pos0, vel0, force_of, mass, node_ptr, 1000, dt, record)
    total, shadow = np.array(total), np.array(shadow)
    assert total.shape == (1001, 3)
    exc = np.abs(total - total[0]).max(0) / total[0]
    drift = np.abs(shadow - shadow[0]).max(0) / shadow[0]
    print("relative excursion of E over 1000 steps", exc, "(bound (omega dt)^2 / 4 = 2.5e-3); of the shadow energy", drift)
    assert (exc > 1e-5).all() and (exc <= 0.1 ** 2 / 4).all()      # it oscillates, within the integrator's band
    assert (drift <= 1e-11).all()                                  # and does not drift
    half = np.abs(total[:500].mean(0) - total[500:1000].mean(0)) / total[0]
    assert (half <= 1e-4).all(), half


# ---------------------------------------------------------------------------------------------
# 4. Langevin on harmonic wells
# ---------------------------------------------------------------------------------------------
LANGEVIN = dict(sizes=[256] * 64, omega_dt=0.5, gamma_dt=0.1, kT=0.7, steps=200, seed=2024)


def langevin_case():
    """16384 independent atoms, 64 structures of 256: (node_ptr, dt [B], gamma [B], mass, k [N, 1], x0)"""
    node_ptr, dt, mass, k, x0, _ = _wells(5, LANGEVIN["sizes"], LANGEVIN["omega_dt"])
    return node_ptr, dt, LANGEVIN["gamma_dt"] / dt, mass, k, x0


def langevin_check(pos, k, x0):
    """<k x^2> = kT per degree of freedom within 5 sqrt(2 / 16384): BAOAB samples the configurations of a harmonic well exactly"""
    n = len(pos)
    assert n == 16384
    got = float((k * (pos - x0) ** 2).mean())
    bound = 5.0 * np.sqrt(2.0 / n)
    print("<k x^2> = %.5f, kT = %.5f: relative deviation %.3e (bound %.3e)" % (got, LANGEVIN["kT"], got / LANGEVIN["kT"] - 1, bound))
    assert abs(got / LANGEVIN["kT"] - 1.0) <= bound


def test_langevin_samples_the_configurations_of_harmonic_wells():
    node_ptr, dt, gamma, mass, k, x0 = langevin_case()
    assert LANGEVIN["steps"] * LANGEVIN["gamma_dt"] >= 10.0        # a time of at least 10 / gamma
    force_of = lambda p: (-k * (p - x0)).astype(np.float32)        # what the device integrator gets
    pos, vel, st = _run(x0.copy(), np.zeros_like(x0), force_of, mass, node_ptr, LANGEVIN["steps"], dt, gamma=gamma, kT=LANGEVIN["kT"],
                        seed=LANGEVIN["seed"], max_disp=1e9)
    langevin_check(pos, k, x0)
    kin = float((mass[:, None] * vel ** 2).mean())
    print("<m v^2> = %.5f (BAOAB's kinetic temperature is low by O((omega dt)^2))" % kin)
    assert 0.8 * LANGEVIN["kT"] <= kin <= 1.02 * LANGEVIN["kT"]


# ---------------------------------------------------------------------------------------------
# 5. / 6. units, arguments
# ---------------------------------------------------------------------------------------------
def test_unit_constants_follow_their_formula():
    from matdeeplearn_amd import forces
    e, amu, k = 1.602176634e-19, 1.66053906660e-27, 1.380649e-23
    unit_time = 1e-10 * np.sqrt(amu / e)                          # seconds: Angstrom sqrt(amu / eV)
    assert forces.EV_A_AMU._fields == ("fs", "kB")
    assert abs(forces.EV_A_AMU.fs * unit_time / 1e-15 - 1.0) <= 1e-15 and abs(forces.EV_A_AMU.kB * e / k - 1.0) <= 1e-15
    assert abs(1.0 / forces.EV_A_AMU.fs - 10.1805) <= 1e-4 and abs(forces.EV_A_AMU.kB - 8.617333e-5) <= 1e-11


def test_md_entry_points_exist_and_check_their_arguments_before_the_library():
    import inspect
    import os
    import re
    from matdeeplearn_amd import _build, _lib, forces, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mdl_hip.h")).read()
    for name in ("mdl_md_step", "mdl_md_velocities"):
        assert name in _lib.PROTOTYPES and re.search(r"\b%s\(" % name, header), name
        if os.path.exists(_build.LIB):
            assert hasattr(_lib.lib(), name), name
    assert len(set(re.findall(r"\b(mdl_[a-z0-9_]+)\s*\(", header))) == 84 == len(_lib.PROTOTYPES)
    assert str(inspect.signature(forces.md)) == (
        "(model, structs, dist_range, masses, dt, steps, kT=0.0, gamma=0.0, kT_init=None, velocities=None, seed=0, fixed=None, "
        "rebuild_every=1, max_disp=0.5, check_every=0, radius=8.0, max_neighbors=12, dictionary=None, output_index=None)")
    assert forces.MDResult._fields == ("positions", "velocities", "energy", "forces", "ekin", "steps", "status", "epot_trace", "ekin_trace",
                                       "node_ptr")
    assert str(inspect.signature(ops.md_step)) == ("(pos, vel, force, mass, node_ptr, state, dt, n_steps, gamma=0.0, kT=0.0, seed=0, "
                                                   "fixed=None, max_disp=0.5)")
    assert str(inspect.signature(ops.md_velocities)) == "(mass, node_ptr, kT, seed=0, fixed=None, zero_momentum=True)"
    pos, ptr = torch.zeros(2, 3, dtype=torch.float64), torch.tensor([0, 2])
    state = ops.MDState(torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.int32), torch.zeros(1, dtype=torch.float64))
    assert [tuple(getattr(state.clone(), k).shape) for k in ("steps", "status", "ekin")] == [(1,)] * 3
    step = lambda st=state, dt=0.1, n=5, **kw: ops.md_step(pos, pos.clone(), torch.zeros(2, 3), torch.ones(2, dtype=torch.float64), ptr, st, dt, n, **kw)
    with pytest.raises(ops.MdlError, match=r"^md_step: state must be an ops\.MDState \(ops\.md_state\)"):
        step(st=None)
    for kw, msg in ((dict(dt=0.0), "dt must be > 0"), (dict(dt=float("nan")), "dt must be > 0"), (dict(gamma=-1.0), "gamma must be >= 0"),
                    (dict(kT=-1e-3), "kT must be >= 0"), (dict(max_disp=0.0), "max_disp must be > 0"), (dict(n=-1), "n_steps must be >= 0")):
        with pytest.raises(ops.MdlError, match="^md_step: " + msg):
            step(**kw)
    with pytest.raises(ops.MdlError, match="^md_velocities: kT must be >= 0"):
        ops.md_velocities(torch.ones(2, dtype=torch.float64), ptr, -1.0)
    with pytest.raises(ops.MdlError, match="HIP device"):            # and the product has no CPU path
        step()
    with pytest.raises(ops.MdlError, match="HIP device"):
        ops.md_velocities(torch.ones(2, dtype=torch.float64), ptr, 1.0)


# ---------------------------------------------------------------------------------------------
# 7. the oracle CGCNN at held lists: the reference trajectory of tests/test_gpu_md.py
# ---------------------------------------------------------------------------------------------
def md_masses(case):
    return np.random.default_rng(21).uniform(1.0, 4.0, len(case.p["pos"]))


def md_initial_velocities(case):
    return md_velocities_reference(md_masses(case), case.p["node_ptr"], MD_KT_INIT, MD_SEED)


def md_reference_trajectory(case, steps, dt, noise=0.0, seed=0):
    """final positions, velocities, prediction and kinetic energy at every evaluation ([steps + 1, B] each) and the largest per-step
    displacement, of `steps` NVE steps in fp64 on the held lists; noise: as test_relax_host.reference_trajectory"""
    rng = np.random.default_rng(seed)
    node_ptr, mass = case.p["node_ptr"], md_masses(case)
    pos, vel, st = case.p["pos"].copy(), md_initial_velocities(case), new_state(len(node_ptr) - 1)
    epot, ekin, step_max = [], [], 0.0
    for _ in range(steps + 1):
        e, f = trh.oracle_energy_forces(case, pos)
        if noise:
            f = f + rng.uniform(-1.0, 1.0, f.shape) * noise * np.abs(f).max()
        pos, vel, st, dg = md_reference(pos, vel, f, mass, node_ptr, st, dt, steps)
        step_max = max([step_max] + [float(d["disp"].max()) for d in dg if len(d["disp"])])
        epot.append(e)
        ekin.append(st["ekin"].copy())
    assert (st["status"] == 1).all() and (st["steps"] == steps).all()
    return pos, vel, np.asarray(epot), np.asarray(ekin), step_max


@functools.lru_cache(maxsize=None)
def cgcnn_md_reference():
    return md_reference_trajectory(trh.cgcnn_case(), **MD_ARGS)


def test_oracle_cgcnn_nve_at_held_lists_energy_excursion_and_noise_sensitivity():
    """50 NVE steps with dt = 1, masses uniform in [1, 4], Maxwell-Boltzmann velocities at kT = 2e-5 (an untrained model's forces are
    of order 1e-3 per A).  Measured here: the atoms travel up to 1.03 A, 0.038 A per step at most (max_disp = 0.5 is far); prediction
    + kinetic energy leaves its first value by 3.8e-7 ... 5.9e-6 per structure (energies of 6.6e-3 ... 2.0e-2), DEV = 3.12e-5 A."""
    case = trh.cgcnn_case()
    pos, vel, epot, ekin, step_max = cgcnn_md_reference()
    moved = np.sqrt(((pos - case.p["pos"]) ** 2).sum(1)).max()
    total = epot + ekin
    exc = np.abs(total - total[0]).max(0)
    print("largest displacement %.3e A, largest step %.3e A; E(0)" % (moved, step_max), total[0], "excursion", exc)
    assert moved >= 0.1 and step_max <= 0.5 - 1e-3
    assert (exc > 0).all() and (exc <= MD_ENERGY_EXCURSION).all() and (exc >= 0.5 * MD_ENERGY_EXCURSION).all()
    noisy = md_reference_trajectory(case, noise=1e-4, seed=1, **MD_ARGS)[0]
    dev = float(np.sqrt(((noisy - pos) ** 2).sum(1)).max())
    print("DEV = %.3e A (MD_TRAJ_BOUND %.1e)" % (dev, MD_TRAJ_BOUND))
    assert 0.0 < dev <= MD_TRAJ_BOUND / 10
