"""Host side of the nudged-elastic-band tests: this file OWNS neb_reference, the fp64 numpy restatement of the band force of
csrc/neb.hip (improved tangent, Henkelman & Jonsson, J. Chem. Phys. 113, 9978; climbing image, 113, 9901) as include/mdl_hip.h
states it for the band mode of mdl_fire_step.  The update of a band is test_relax_host.fire_reference called with the band as one
structure.  Here: an analytic saddle point, every branch of the definition on hand-computable cases, the public surface, and the
fp64 reference trajectory of the oracle CGCNN at held neighbour lists that tests/test_gpu_neb.py compares forces.neb with.  The
upstream reference has no counterpart, so no golden from it exists.  No GPU.

NEB_TRAJ_BOUND, the bound of that comparison, is the reference's own sensitivity: the same 20 band steps with every force
component perturbed by uniform noise of amplitude 1e-4 max|F| moved the final positions by DEV = 3.34e-5 A at most (measured
here; the atoms travel up to 0.62 A); NEB_TRAJ_BOUND = 10 x DEV, rounded up to two digits, by the project's "measured x 10"
rule, as TRAJ_BOUND and MD_TRAJ_BOUND were set."""
import functools
import inspect
import types

import numpy as np
import pytest
import torch

import test_gpu_forces as tgf
import test_relax_host as trh

NEB_TRAJ_BOUND = 3.4e-4           # A; 10 x the DEV measured below (see the module docstring)


def _adjugate(m):
    """row-major 3x3: (adjugate, determinant), the expressions of csrc/struct_reduce.h"""
    m = np.asarray(m, dtype=np.float64).reshape(9)
    adj = np.array([m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                    m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                    m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]])
    return adj, m[0] * adj[0] + m[1] * adj[3] + m[2] * adj[6]


def min_image(d, cell, pbc):
    """d [n, 3] wrapped to its minimum image in `cell` (rows are lattice vectors) on the axes whose bit is set in pbc.  Returns
    (d, the smallest distance of a rounded fractional coordinate from a half: how marginal the rounding was)"""
    adj, det = _adjugate(cell)
    pb = int(pbc) & 7
    if det == 0.0 or pb == 0:
        return d, 0.5
    inv, C = (adj / det).reshape(3, 3), np.asarray(cell, dtype=np.float64).reshape(3, 3)
    f = np.stack([d[:, 0] * inv[0, k] + d[:, 1] * inv[1, k] + d[:, 2] * inv[2, k] for k in range(3)], 1)
    margin = 0.5
    for k in range(3):
        if pb >> k & 1:
            if len(f):
                margin = min(margin, float(np.abs(np.abs(f[:, k] - np.floor(f[:, k])) - 0.5).min()))
            f[:, k] -= np.rint(f[:, k])
    return np.stack([f[:, 0] * C[0, k] + f[:, 1] * C[1, k] + f[:, 2] * C[2, k] for k in range(3)], 1), margin


def band_climber(energy, i0, i1, climb):
    """the interior image of largest energy, lowest index on ties; -1 without an interior image or without climbing"""
    if not climb or i1 - i0 < 3:
        return -1
    return i0 + 1 + int(np.argmax(np.asarray(energy[i0 + 1:i1 - 1])))         # argmax: the first of equal maxima


def neb_reference(pos, force, energy, image_ptr, band_ptr, cell, pbc, spring, climb, fixed=None):
    """The band force of every image, fp64.  pos [N, 3]; force [N, 3] and energy [I] are taken as the fp32 values given; cell
    [I, 3, 3]; pbc [I] bit masks; spring, climb [B].  Returns (band_force [N, 3] float64 — NOT yet rounded to fp32 —, tangent_force
    [I], seg_len [I], climber [B] int32, diag): diag[s] holds what the decisions of image s were taken from (role, the relative
    gaps of the energies compared, the margin of the wrap)."""
    pos = np.asarray(pos, dtype=np.float64)
    force = np.asarray(force, dtype=np.float32).astype(np.float64)
    energy = np.asarray(energy, dtype=np.float32).astype(np.float64)
    N, I, B = len(pos), len(image_ptr) - 1, len(band_ptr) - 1
    free = np.ones(N, bool) if fixed is None else ~np.asarray(fixed).astype(bool)
    out, ft_all, seg = np.zeros((N, 3)), np.zeros(I), np.zeros(I)
    climber, diag = np.full(B, -1, np.int32), [None] * I
    for b in range(B):
        i0, i1 = int(band_ptr[b]), int(band_ptr[b + 1])
        climber[b] = band_climber(energy, i0, i1, climb[b])
        for s in range(i0, i1):
            a0, a1 = int(image_ptr[s]), int(image_ptr[s + 1])
            n = a1 - a0
            R = pos[a0:a1]
            d = diag[s] = {"role": "end", "gaps": [], "wrap": 0.5}
            tm = tp = np.zeros((n, 3))
            if s > i0:
                tm, w = min_image(R - pos[a0 - n:a0], cell[s], pbc[s])
                d["wrap"] = min(d["wrap"], w)
                seg[s] = np.sqrt((tm * tm).sum())
            if s == i0 or s == i1 - 1:
                continue
            tp, w = min_image(pos[a1:a1 + n] - R, cell[s], pbc[s])
            d["wrap"] = min(d["wrap"], w)
            F = np.where(free[a0:a1, None], force[a0:a1], 0.0)
            Ep, E0, En = energy[s - 1], energy[s], energy[s + 1]
            rel = lambda x, y: abs(x - y) / max(abs(x), abs(y)) if x != y else 0.0
            d["gaps"] = [rel(En, E0), rel(E0, Ep), rel(En, Ep)]
            if En > E0 > Ep:
                ca, cb, d["role"] = 1.0, 0.0, "up"
            elif En < E0 < Ep:
                ca, cb, d["role"] = 0.0, 1.0, "down"
            else:
                hi, lo = max(abs(En - E0), abs(Ep - E0)), min(abs(En - E0), abs(Ep - E0))
                d["gaps"].append(rel(abs(En - E0), abs(Ep - E0)))
                (ca, cb), d["role"] = ((hi, lo), "extremum-up") if En > Ep else ((lo, hi), "extremum-down")
            pp, mm, pm = (tp * tp).sum(), (tm * tm).sum(), (tp * tm).sum()
            t2 = ca * ca * pp + 2.0 * ca * cb * pm + cb * cb * mm
            if not t2 > 0.0:
                d["role"] += ", no tangent"
                out[a0:a1] = F
                continue
            lt = np.sqrt(t2)
            tau = (ca * tp + cb * tm) / lt
            ft = (ca * (F * tp).sum() + cb * (F * tm).sum()) / lt
            ft_all[s] = ft
            if climber[b] == s:
                d["role"] += ", climber"
                g = -2.0 * ft
            else:
                g = spring[b] * (np.sqrt(pp) - np.sqrt(mm)) - ft
            out[a0:a1] = np.where(free[a0:a1, None], F + g * tau, 0.0)
    return out, ft_all, seg, climber, diag


def neb_step_reference(pos, vel, force, energy, image_ptr, band_ptr, cell, pbc, spring, climb, state, fmax, fixed=None, **constants):
    """neb_reference, its force rounded to fp32 once, then fire_reference with every band as one structure; the end images are
    fixed.  Returns (pos, vel, state, band_force fp32, tangent_force, seg_len, climber)"""
    N = len(pos)
    mask = np.zeros(N, bool) if fixed is None else np.asarray(fixed).astype(bool).copy()
    for b in range(len(band_ptr) - 1):
        if band_ptr[b + 1] > band_ptr[b]:
            for s in (band_ptr[b], band_ptr[b + 1] - 1):
                mask[image_ptr[s]:image_ptr[s + 1]] = True
    bf, ft, seg, climber, _ = neb_reference(pos, force, energy, image_ptr, band_ptr, cell, pbc, spring, climb, mask)
    bf = bf.astype(np.float32)
    node_ptr = np.asarray(image_ptr)[np.asarray(band_ptr)]
    pos, vel, st, _ = trh.fire_reference(pos, vel, bf, node_ptr, state, fmax, mask, **constants)
    return pos, vel, st, bf, ft, seg, climber


# ---------------------------------------------------------------------------------------------
# 1. an analytic saddle point
# ---------------------------------------------------------------------------------------------
def _V(p):
    """V = (x^2 - 1)^2 + 5 (y - 0.3 (1 - x^2))^2 + 5 z^2: minima (+-1, 0, 0) with V = 0, saddle (0, 0.3, 0) with V = 1, a curved path"""
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    u = y - 0.3 * (1.0 - x * x)
    V = (x * x - 1.0) ** 2 + 5.0 * u * u + 5.0 * z * z
    F = -np.stack([4.0 * x * (x * x - 1.0) + 6.0 * x * u, 10.0 * u, 10.0 * z], 1)
    return V, F


def _run_saddle(start, max_steps=200, spring=1.0, dt=0.02, dt_max=0.2, fmax=1e-4):
    """one-atom images from `start` [n, 3]; climbing from step 0; forces and energies rounded to fp32 as the device gets them"""
    n = len(start)
    image_ptr, band_ptr = np.arange(n + 1), np.array([0, n])
    cell, pbc = np.zeros((n, 3, 3)), np.zeros(n, np.int32)
    pos, vel, st = start.copy(), np.zeros_like(start), trh.new_state(1, dt=dt)
    for it in range(max_steps + 1):
        V, F = _V(pos)
        pos, vel, st, bf, ft, seg, climber = neb_step_reference(pos, vel, F.astype(np.float32), V.astype(np.float32), image_ptr, band_ptr,
                                                                cell, pbc, [spring], [1], st, fmax, dt_max=dt_max)
        if st["done"][0]:
            break
    return pos, st, seg, int(climber[0])


def _straight(n, x0=-1.0, x1=1.0):
    start = np.zeros((n, 3))
    start[:, 0] = np.linspace(x0, x1, n)
    start[1:-1, 2] = 0.05                                       # off the plane of the path: z has to relax too
    return start


@pytest.mark.parametrize("n_images", [5, 7])
def test_band_finds_the_analytic_saddle(n_images):
    pos, st, seg, climber = _run_saddle(_straight(n_images))
    e = _V(pos)[0]
    print("%d images: %d steps, climber %d at %s, E - 1 = %.2e, segments %s" % (n_images, st["steps"][0], climber, pos[climber], e[climber] - 1.0,
                                                                              seg[1:]))
    assert st["done"][0] == 1 and st["steps"][0] <= 200
    assert climber == n_images // 2
    assert abs(e[climber] - 1.0) <= 1e-6
    assert np.abs(pos[climber] - [0.0, 0.3, 0.0]).max() <= 1e-3
    assert np.abs(seg[1:] / seg[1:].mean() - 1.0).max() <= 0.01


@functools.lru_cache(maxsize=None)
def _relaxed_path():
    return _run_saddle(_straight(7))[0]


def test_asymmetric_band_finds_the_same_saddle():
    """End points (-1, 0, 0) and the image at x = 0.6 of the relaxed 7-image path (its sixth image), 7 images, the settings of the
    symmetric bands.  The climber feels no spring, so at convergence every other interior image sits midway between its
    neighbours: the segments are equal on either side of the climber, and the two sides differ — equal spacing is asserted
    per side."""
    path = _relaxed_path()
    end = path[5]
    assert abs(end[0] - 0.6) < 0.1, end
    start = np.linspace(0.0, 1.0, 7)[:, None] * (end - path[0])[None, :] + path[0][None, :]
    start[1:-1, 2] += 0.05
    pos, st, seg, climber = _run_saddle(start)
    e = _V(pos)[0]
    print("asymmetric: %d steps, climber %d at %s, E - 1 = %.2e, segments %s" % (st["steps"][0], climber, pos[climber], e[climber] - 1.0, seg[1:]))
    assert st["done"][0] == 1 and st["steps"][0] <= 200
    assert abs(e[climber] - 1.0) <= 1e-6
    assert np.abs(pos[climber] - [0.0, 0.3, 0.0]).max() <= 1e-3
    for side in (seg[1:climber + 1], seg[climber + 1:]):
        assert len(side) >= 1 and np.abs(side / side.mean() - 1.0).max() <= 0.01, seg


# ---------------------------------------------------------------------------------------------
# 2. every branch of the definition on hand-computable cases
# ---------------------------------------------------------------------------------------------
def _one_band(points, energies, F_mid=(2.0, 1.0, 0.0), spring=0.5, climb=0, cell=None, pbc=0, fixed=None):
    """one-atom images at `points`; every interior image feels F_mid.  Returns neb_reference's result"""
    n = len(points)
    pos = np.asarray(points, dtype=np.float64)
    force = np.tile(np.asarray(F_mid, np.float32), (n, 1))
    cells = np.zeros((n, 3, 3)) if cell is None else np.tile(np.asarray(cell, np.float64), (n, 1, 1))
    return neb_reference(pos, force, np.asarray(energies, np.float32), np.arange(n + 1), [0, n], cells, np.full(n, pbc, np.int32), [spring],
                         [climb], fixed)


CORNER = [(0.0, 0.0, 0.0), (1.0, 0.0, 0.0), (1.0, 2.0, 0.0)]          # t- = (1, 0, 0), t+ = (0, 2, 0): |t+| - |t-| = 1


def test_the_four_tangent_cases_and_the_tie_by_hand():
    F, k = np.array([2.0, 1.0, 0.0]), 0.5
    r17, r2, r5 = np.sqrt(17.0), np.sqrt(2.0), np.sqrt(5.0)
    cases = {
        # energies: (role, tangent, F.t^)
        (0, 1, 2): ("up", np.array([0.0, 1.0, 0.0]), 1.0),
        (2, 1, 0): ("down", np.array([1.0, 0.0, 0.0]), 2.0),
        (0, 2, 1): ("extremum-up", np.array([1.0, 4.0, 0.0]) / r17, 6.0 / r17),        # (hi, lo) = (2, 1): t = 2 t+ + t-
        (2, 0, 1): ("extremum-down", np.array([1.0, 1.0, 0.0]) / r2, 3.0 / r2),        # (lo, hi) = (1, 2): t = t+ + 2 t-
        (1, 0, 1): ("extremum-down", np.array([1.0, 2.0, 0.0]) / r5, 4.0 / r5),        # the tie: (lo, hi) = (1, 1)
    }
    for energies, (role, tau, ft) in cases.items():
        bf, tf, seg, climber, diag = _one_band(CORNER, energies, spring=k)
        assert diag[1]["role"] == role, (energies, diag[1])
        want = F - ft * tau + k * (2.0 - 1.0) * tau
        assert np.allclose(bf[1], want, rtol=0, atol=1e-14), (energies, bf[1], want)
        assert abs(tf[1] - ft) <= 1e-14 and tf[0] == 0 and tf[2] == 0
        assert np.array_equal(seg, [0.0, 1.0, 2.0]) and climber[0] == -1
        assert not bf[0].any() and not bf[2].any()                               # the end images: zero rows
    # the climbing image: the maximum, the tangent component inverted, no spring
    bf, tf, seg, climber, diag = _one_band(CORNER, (0, 2, 1), climb=1)
    tau, ft = np.array([1.0, 4.0, 0.0]) / r17, 6.0 / r17
    assert climber[0] == 1 and "climber" in diag[1]["role"]
    assert np.allclose(bf[1], F - 2.0 * ft * tau, rtol=0, atol=1e-14) and abs(tf[1] - ft) <= 1e-14


def test_climber_tie_coinciding_images_short_bands_and_fixed_atoms_by_hand():
    line = [(float(i), 0.0, 0.0) for i in range(5)]
    # two interior images share the largest energy: the lower index climbs; climb = 0: nobody
    assert _one_band(line, (0, 2, 1, 2, 0), climb=1)[3][0] == 1
    assert _one_band(line, (0, 1, 2, 2, 0), climb=1)[3][0] == 2
    assert _one_band(line, (0, 2, 1, 2, 0), climb=0)[3][0] == -1
    assert _one_band(line, (9, 2, 1, 3, 9), climb=1)[3][0] == 3                # the end images never climb
    # coinciding images: "up" takes t+ alone, and t+ = 0 -> the true force, no tangent force
    bf, tf, seg, _, diag = _one_band([(0, 0, 0), (1, 0, 0), (1, 0, 0)], (0, 1, 2))
    assert "no tangent" in diag[1]["role"] and np.array_equal(bf[1], [2.0, 1.0, 0.0]) and tf[1] == 0 and np.array_equal(seg, [0, 1, 0])
    # a band of two images, and of one: no interior image, zero rows, the segment length still there
    bf, tf, seg, climber, _ = _one_band([(0, 0, 0), (3, 4, 0)], (0, 1), climb=1)
    assert not bf.any() and not tf.any() and np.array_equal(seg, [0.0, 5.0]) and climber[0] == -1
    bf, tf, seg, climber, _ = _one_band([(0, 0, 0)], (0,), climb=1)
    assert not bf.any() and seg[0] == 0 and climber[0] == -1
    # fixed atoms: two atoms per image, the second fixed — its force counts as zero in F.t^, its row is zero, its displacement
    # still belongs to the tangent
    pos = np.array([[0, 0, 0], [5, 0, 0], [1, 0, 0], [5, 1, 0], [2, 0, 0], [5, 2, 0]], dtype=np.float64)
    force = np.tile(np.array([[2.0, 1.0, 0.0], [7.0, 7.0, 7.0]], np.float32), (3, 1))
    fixed = np.array([0, 1] * 3)
    bf, tf, seg, _, _ = neb_reference(pos, force, np.array([0, 1, 2], np.float32), [0, 2, 4, 6], [0, 3], np.zeros((3, 3, 3)), np.zeros(3, np.int32),
                                      [0.5], [0], fixed)
    tau = np.array([[1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]) / np.sqrt(2.0)             # t+ over both atoms, |t+| = |t-| = sqrt 2
    ft = 2.0 / np.sqrt(2.0)
    assert abs(tf[1] - ft) <= 1e-14 and np.allclose(bf[2], np.array([2.0, 1.0, 0.0]) - ft * tau[0], rtol=0, atol=1e-14)
    assert not bf[3].any() and np.allclose(seg, [0, np.sqrt(2.0), np.sqrt(2.0)])


def test_minimum_image_in_a_triclinic_cell_and_a_non_periodic_axis_by_hand():
    cell = np.array([[4.0, 0.0, 0.0], [1.0, 5.0, 0.0], [0.5, 0.5, 6.0]])
    # the middle image sits just inside the face spanned by b and c; the next image has crossed it and been wrapped back by -a
    pts = np.array([(3.7, 1.0, 1.0), (3.9, 1.0, 1.0), (4.1, 1.0, 1.0)])
    wrapped = pts.copy()
    wrapped[2] -= cell[0]
    for pbc, crossed in ((7, False), (1, False), (6, True), (0, True)):           # periodic along a: the crossing is undone
        bf, tf, seg, _, diag = _one_band(wrapped, (0, 1, 2), cell=cell, pbc=pbc)
        want_tp = np.array([-3.8, 0.0, 0.0]) if crossed else np.array([0.2, 0.0, 0.0])
        tau = want_tp / np.linalg.norm(want_tp)
        ft = float(np.array([2.0, 1.0, 0.0]) @ tau)
        want = np.array([2.0, 1.0, 0.0]) - ft * tau + 0.5 * (np.linalg.norm(want_tp) - 0.2) * tau
        assert np.allclose(bf[1], want, rtol=0, atol=1e-13), (pbc, bf[1], want)
        assert abs(seg[1] - 0.2) <= 1e-14 and abs(seg[2] - np.linalg.norm(want_tp)) <= 1e-13
        assert diag[1]["wrap"] > 0.4 or pbc == 0
    # a shift by the lattice vector b changes x AND y (triclinic); it is undone only where axis b is periodic
    wrapped = pts.copy()
    wrapped[2] += cell[1]
    assert abs(_one_band(wrapped, (0, 1, 2), cell=cell, pbc=2)[2][2] - 0.2) <= 1e-13
    assert abs(_one_band(wrapped, (0, 1, 2), cell=cell, pbc=5)[2][2] - np.linalg.norm(cell[1] + [0.2, 0, 0])) <= 1e-13
    # a cell without volume: no wrap, whatever pbc says
    flat = np.array([[4.0, 0.0, 0.0], [1.0, 5.0, 0.0], [5.0, 5.0, 0.0]])
    assert abs(_one_band(wrapped, (0, 1, 2), cell=flat, pbc=7)[2][2] - np.linalg.norm(cell[1] + [0.2, 0, 0])) <= 1e-13


# the batch of tests/test_gpu_neb.py: every role of the band force and of the update in one launch
#         images, atoms per image, energies (exact fp32 values: compared energies are equal or far apart), pbc, climb
BANDS = [(2, 1, (0, 1), 0, 1),                                     # no interior image: zero rows, FIRE latches it
         (3, 2, (0, 1, 2), 0, 1),                                  # the interior image coincides with the next one: F_band = F
         (5, 63, (0, 1, 3, 2, 0.5), 7, 1),                         # up, the climber (an extremum), down; triclinic, a face crossed
         (9, 64, (0, 1, 2, 1, 0.5, 1.25, 2, 1.5, 0), 3, 1),        # the energy tie at 2, the climber tie 2 / 6, a minimum; z open
         (5, 65, (1, 3, 0.5, 2, 0), 7, 0),                         # no climbing; extrema with E(i+1) < E(i-1)
         (3, 257, (0, 1, 2), 7, 1),                                # latched before; a cell without volume
         (3, 513, (2, 1, 0), 5, 1)]                                # converges in this call
TWO, COINCIDE, TRICLINIC, TIES, NOCLIMB, LATCHED, CONVERGING = range(7)


@functools.lru_cache(maxsize=None)
def neb_batch():
    rng = np.random.default_rng(7)
    n_img = [b[0] for b in BANDS]
    band_ptr = np.concatenate([[0], np.cumsum(n_img)]).astype(np.int64)
    counts = np.repeat([b[1] for b in BANDS], n_img)
    image_ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    I, B, N = len(counts), len(BANDS), int(image_ptr[-1])
    energy = np.concatenate([np.asarray(b[2], np.float32) for b in BANDS])
    pbc = np.repeat([b[3] for b in BANDS], n_img).astype(np.int32)
    tri = np.array([[7.0, 0.0, 0.0], [1.5, 8.0, 0.0], [-1.0, 2.0, 9.0]])
    band_cell = [np.zeros((3, 3)), np.zeros((3, 3)), tri, tri * 1.1, np.diag([6.0, 7.0, 8.0]), np.array([[4.0, 0, 0], [0, 5.0, 0], [4.0, 5.0, 0]]),
                 tri[[1, 2, 0]]]
    cell = np.concatenate([np.tile(band_cell[b], (n_img[b], 1, 1)) for b in range(B)])
    pos = np.zeros((N, 3))
    for b in range(B):
        n = BANDS[b][1]
        base, step = rng.uniform(0.0, 6.0, (n, 3)), 0.1 * rng.normal(size=(n, 3))
        for k, s in enumerate(range(band_ptr[b], band_ptr[b + 1])):
            pos[image_ptr[s]:image_ptr[s + 1]] = base + k * step + 0.02 * rng.normal(size=(n, 3))
    s = band_ptr[COINCIDE] + 1                                    # the interior image of COINCIDE sits on the last one
    pos[image_ptr[s]:image_ptr[s + 1]] = pos[image_ptr[s + 1]:image_ptr[s + 2]]
    s = band_ptr[TRICLINIC] + 2                                   # atom 0 of image 2 went through a face and was wrapped back
    pos[image_ptr[s]] -= tri[0]
    pos[image_ptr[s] + 1] += tri[1] - tri[2]
    s = band_ptr[TIES] + 4                                        # a whole lattice vector along the OPEN axis: not undone
    pos[image_ptr[s] + 1] += 1.1 * tri[2]
    pos[image_ptr[s] + 2] += 1.1 * tri[0]                          # and along a periodic one: undone
    force = (0.3 * rng.normal(size=(N, 3))).astype(np.float32)
    fixed = np.zeros(N, np.uint8)
    for b in (TRICLINIC, NOCLIMB):                                # the same atoms of every image of the band
        for s in range(band_ptr[b], band_ptr[b + 1]):
            fixed[image_ptr[s]:image_ptr[s + 1]][::5] = 1
    spring = np.array([1.0, 1.0, 0.5, 2.0, 1.0, 1.0, 1.0])
    climb = np.array([b[4] for b in BANDS], np.uint8)
    st = trh.new_state(B)
    st["dt"] = np.array([0.1, 0.1, 0.2, 0.95, 0.3, 0.1, 0.2])
    st["alpha"] = np.array([0.1, 0.1, 0.07, 0.09, 0.05, 0.1, 0.1])
    st["n_pos"] = np.array([0, 0, 2, 7, 4, 0, 3], np.int32)
    st["steps"] = np.array([0, 0, 12, 9, 30, 4, 4], np.int32)    # COINCIDE makes its first step
    st["done"][LATCHED] = 1
    st["fmax_seen"][:] = -1.0
    fmax = np.full(B, 0.05)
    fmax[CONVERGING] = 100.0
    # velocities along the band force (F.v > 0: mixing, TIES accelerates into the dt clamp), against it in NOCLIMB (reset)
    mask = fixed.astype(bool)
    bf = neb_reference(pos, force, energy, image_ptr, band_ptr, cell, pbc, spring, climb, mask)[0]
    sign = np.ones(N)
    sign[image_ptr[band_ptr[NOCLIMB]]:image_ptr[band_ptr[NOCLIMB + 1]]] = -1.0
    vel = sign[:, None] * (bf + 0.05 * rng.normal(size=(N, 3))) * 0.7
    return types.SimpleNamespace(pos=pos, vel=vel, force=force, energy=energy, image_ptr=image_ptr, band_ptr=band_ptr, cell=cell, pbc=pbc,
                                 spring=spring, climb=climb, state=st, fmax=fmax, fixed=fixed, I=I, B=B, N=N)


def sub_batch(c, b):
    """band b of the batch alone: the same namespace with one band"""
    i0, i1 = int(c.band_ptr[b]), int(c.band_ptr[b + 1])
    a0, a1 = int(c.image_ptr[i0]), int(c.image_ptr[i1])
    st = {k: v[b:b + 1].copy() for k, v in c.state.items()}
    return types.SimpleNamespace(pos=c.pos[a0:a1].copy(), vel=c.vel[a0:a1].copy(), force=c.force[a0:a1].copy(), energy=c.energy[i0:i1].copy(),
                                 image_ptr=c.image_ptr[i0:i1 + 1] - a0, band_ptr=np.array([0, i1 - i0], np.int64), cell=c.cell[i0:i1].copy(),
                                 pbc=c.pbc[i0:i1].copy(), spring=c.spring[b:b + 1].copy(), climb=c.climb[b:b + 1].copy(), state=st,
                                 fmax=c.fmax[b:b + 1].copy(), fixed=c.fixed[a0:a1].copy(), I=i1 - i0, B=1, N=a1 - a0, rows=slice(a0, a1),
                                 images=slice(i0, i1))


def test_the_batch_of_the_gpu_test_holds_every_role_and_no_marginal_decision():
    c = neb_batch()
    mask = c.fixed.astype(bool).copy()
    for b in range(c.B):
        for s in (c.band_ptr[b], c.band_ptr[b + 1] - 1):
            mask[c.image_ptr[s]:c.image_ptr[s + 1]] = True
    bf, tf, seg, climber, diag = neb_reference(c.pos, c.force, c.energy, c.image_ptr, c.band_ptr, c.cell, c.pbc, c.spring, c.climb, mask)
    roles = [d["role"] for d in diag]
    img = lambda b, k: roles[c.band_ptr[b] + k]
    assert roles[:2] == ["end", "end"] and img(COINCIDE, 1) == "up, no tangent"
    assert [img(TRICLINIC, k) for k in range(5)] == ["end", "up", "extremum-up, climber", "down", "end"]
    assert [img(TIES, k) for k in range(1, 8)] == ["up", "extremum-down, climber", "down", "extremum-up", "up", "extremum-up", "down"]
    assert [img(NOCLIMB, k) for k in range(1, 4)] == ["extremum-down", "extremum-down", "extremum-down"]
    assert list(climber) == [-1, c.band_ptr[COINCIDE] + 1, c.band_ptr[TRICLINIC] + 2, c.band_ptr[TIES] + 2, -1, c.band_ptr[LATCHED] + 1,
                             c.band_ptr[CONVERGING] + 1]
    assert {b[1] for b in BANDS} == {1, 2, 63, 64, 65, 257, 513} and {b[0] for b in BANDS} == {2, 3, 5, 9}
    for d in diag:
        assert all(g == 0.0 or g >= 1e-3 for g in d["gaps"]), d           # energies: equal fp32 values or far apart
        assert d["wrap"] >= 1e-3, d                                         # no fractional coordinate near a half
    # the wraps happened: the crossing atoms of TRICLINIC have short displacements, the open axis of TIES keeps its long one
    s = c.band_ptr[TRICLINIC] + 2
    assert seg[s] < 3.0 and seg[s + 1] < 3.0
    s = c.band_ptr[TIES] + 4
    assert 9.0 < seg[s] < 12.5 and 9.0 < seg[s + 1] < 12.5
    # the update: every branch, no marginal decision (the rule of tests/test_gpu_relax.py)
    out = neb_step_reference(c.pos, c.vel, c.force, c.energy, c.image_ptr, c.band_ptr, c.cell, c.pbc, c.spring, c.climb, c.state, c.fmax, c.fixed)
    node_ptr = c.image_ptr[c.band_ptr]
    _, _, rst, fd = trh.fire_reference(c.pos, c.vel, out[3], node_ptr, c.state, c.fmax, mask)
    assert [d["branch"] for d in fd] == ["converged", "first", "uphill-free", "accelerate", "reset", "converged", "converged"]
    assert fd[TWO]["fm"] == 0 and fd[CONVERGING]["fm"] > 0 and rst["dt"][TIES] == trh.FIRE_CONSTANTS["dt_max"]
    mx = trh.FIRE_CONSTANTS["maxstep"]
    for b, d in enumerate(fd):
        if d["branch"] not in ("converged", "first"):
            assert abs(d["P"]) >= 1e-3 * d["abs_fv"], (b, d)
        if d["branch"] != "converged":
            assert abs(d["s"] - mx) >= 1e-3 * mx, (b, d)
        if not c.state["done"][b] and d["fm"] > 0:
            assert abs(d["fm"] - c.fmax[b]) >= 1e-3 * c.fmax[b], (b, d)
    assert {d["s"] > mx for d in fd if d["branch"] != "converged"} == {True, False}       # the clip active and inactive


# ---------------------------------------------------------------------------------------------
# 3. the surface
# ---------------------------------------------------------------------------------------------
def test_surface_signatures_and_argument_errors_before_the_library():
    import os
    import re
    from matdeeplearn_amd import _lib, forces, ops
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "mdl_hip.h")).read()
    assert re.search(r"\bmdl_fire_step\(", header) and "image_ptr" in header and "mdl_fire_step" in _lib.PROTOTYPES
    assert len(_lib.PROTOTYPES) == 84 == len(set(re.findall(r"\b(mdl_[a-z0-9_]+)\s*\(", header)))
    assert len(_lib.PROTOTYPES["mdl_fire_step"][1]) == 34                         # 22 of the plain call + 12 of the band mode
    assert str(inspect.signature(forces.neb)) == (
        "(model, bands, dist_range, fmax=0.05, steps=200, spring=1.0, climb=True, climb_after=0, rebuild_every=1, fixed=None, dt=0.1, "
        "dt_max=1.0, maxstep=0.2, n_min=5, f_inc=1.1, f_dec=0.5, alpha=0.1, f_alpha=0.99, check_every=10, radius=8.0, max_neighbors=12, "
        "dictionary=None, output_index=None)")
    assert str(inspect.signature(ops.neb_step)) == "(pos, vel, force, energy, cell, pbc, state, fmax, spring=1.0, climb=True, **constants)"
    assert str(inspect.signature(ops.neb_state)) == "(image_ptr, band_ptr, fixed=None, dt=0.1, alpha=0.1)"
    assert str(inspect.signature(ops.fire_step)) == "(pos, vel, force, node_ptr, state, fmax, fixed=None, **constants)"
    assert forces.NEBResult._fields == ("positions", "energy", "forces", "band_forces", "converged", "steps", "fmax", "climber", "barrier",
                                        "tangent_force", "path", "node_ptr", "band_ptr")
    assert ops.NebState.__slots__[:6] == ops.FireState.__slots__
    assert set(ops.NebState.__slots__[6:]) == {"image_ptr", "band_ptr", "band_node_ptr", "fixed", "climber", "tangent_force", "seg_len", "band_force"}
    # argument errors come before a device or the library is asked for anything
    loaded = _lib._lib
    z = lambda *s: torch.zeros(*s, dtype=torch.float64)
    with pytest.raises(ops.MdlError, match="HIP device"):
        ops.neb_state(torch.tensor([0, 1, 2, 3]), torch.tensor([0, 3]))
    with pytest.raises(ops.MdlError, match="neb_step: state must be an ops.NebState"):
        ops.neb_step(z(3, 3), z(3, 3), torch.zeros(3, 3), torch.zeros(3), z(3, 3, 3), torch.zeros(3, dtype=torch.int32),
                     ops.FireState(*[torch.zeros(1)] * 6), 0.05)
    state = ops.NebState(*[torch.zeros(1)] * 14)
    with pytest.raises(ops.MdlError, match="HIP device"):
        ops.neb_step(z(3, 3), z(3, 3), torch.zeros(3, 3), torch.zeros(3), z(3, 3, 3), torch.zeros(3, dtype=torch.int32), state, 0.05)
    with pytest.raises(ops.MdlError, match="NebState: 14 fields"):
        ops.NebState(torch.zeros(1))
    assert _lib._lib is loaded


def test_interpolate_band_is_linear_in_the_minimum_image_displacement():
    from matdeeplearn_amd import forces, ops
    cell = np.array([[4.0, 0.0, 0.0], [1.0, 5.0, 0.0], [0.5, 0.5, 6.0]])
    a = {"positions": np.array([[3.9, 1.0, 1.0], [1.0, 1.0, 1.0]]), "numbers": np.array([3, 8]), "cell": cell, "pbc": [True, True, False]}
    b = dict(a, positions=np.array([[0.1, 1.0, 1.0], [1.0, 1.4, 1.0 + 6.0]]))        # atom 0 crossed the face; atom 1 moved along open c
    band = forces.interpolate_band(a, b, 5)
    assert len(band) == 5 and np.array_equal(band[0]["positions"], a["positions"])
    for k, s in enumerate(band):
        assert np.allclose(s["positions"][0], [3.9 + 0.05 * k, 1.0, 1.0], atol=1e-13)      # through the face, not back across the cell
        assert np.allclose(s["positions"][1], [1.0, 1.0 + 0.1 * k, 1.0 + 1.5 * k], atol=1e-13)
        assert np.array_equal(s["numbers"], a["numbers"]) and np.array_equal(s["cell"], cell) and s["pbc"] == a["pbc"]
    assert len(forces.interpolate_band(a, b, 2)) == 2
    for bad in (dict(b, positions=b["positions"][:1], numbers=b["numbers"][:1]), dict(b, numbers=np.array([3, 9])), dict(b, cell=cell * 1.01),
                dict(b, pbc=[True, True, True])):
        with pytest.raises(ops.MdlError, match="interpolate_band"):
            forces.interpolate_band(a, bad, 5)
    with pytest.raises(ops.MdlError, match="n_images"):
        forces.interpolate_band(a, b, 1)


# ---------------------------------------------------------------------------------------------
# 4. the oracle CGCNN at held lists: the reference trajectory of tests/test_gpu_neb.py
# ---------------------------------------------------------------------------------------------
NEB_ARGS = dict(steps=20, dt=3.0, dt_max=30.0, fmax=0.0, spring=0.01)
NEB_IMAGES, NEB_PICK, NEB_NOISE = 5, (0, 1), 0.3


@functools.lru_cache(maxsize=None)
def neb_case():
    """Two bands of NEB_IMAGES images: two bulk structures of test_relax_host.cgcnn_case and copies displaced by uniform noise of
    NEB_NOISE A (seeded), interpolated by forces.interpolate_band; host-built graphs of every image (held throughout) and that
    case's fp64 oracle CGCNN (its weights and settings)."""
    from matdeeplearn_amd import forces
    from matdeeplearn_amd.process import graph as pg
    base = trh.cgcnn_case()
    rng = np.random.default_rng(3)
    bands = []
    for i in NEB_PICK:
        s = base.structs[i]
        final = dict(s, positions=s["positions"] + rng.uniform(-NEB_NOISE, NEB_NOISE, s["positions"].shape))
        bands.append(forces.interpolate_band(s, final, NEB_IMAGES))
    structs = [s for band in bands for s in band]
    p = tgf._pack(structs)
    xs, src, tgt = [], [], []
    for b, s in enumerate(structs):
        g = pg.build_graph(s["positions"], s["numbers"], s["cell"], s["pbc"])
        ei = pg.sort_by_target(g["edge_index"])[0] + p["node_ptr"][b]
        xs.append(g["x"])
        src.append(ei[0])
        tgt.append(ei[1])
    batch = torch.from_numpy(np.repeat(np.arange(len(structs)), np.diff(p["node_ptr"])))
    band_ptr = np.arange(len(bands) + 1, dtype=np.int64) * NEB_IMAGES
    return types.SimpleNamespace(bands=bands, structs=structs, p=p, x=torch.from_numpy(np.concatenate(xs)).double(), src=np.concatenate(src),
                                 tgt=np.concatenate(tgt), batch=batch, model=base.model, state_dict=base.state_dict, band_ptr=band_ptr)


def neb_reference_trajectory(case, steps, dt, dt_max, fmax, spring, noise=0.0, seed=0):
    """positions, state, climbers and per-step diagnostics of `steps` band steps in fp64, climbing from step 0; noise: every force
    component perturbed by uniform noise of amplitude noise * max|F| before the band force sees it"""
    rng = np.random.default_rng(seed)
    p, B = case.p, len(case.band_ptr) - 1
    pos, vel, st = p["pos"].copy(), np.zeros_like(p["pos"]), trh.new_state(B, dt=dt)
    log = []
    for _ in range(steps):
        e, f = trh.oracle_energy_forces(case, pos)
        if noise:
            f = f + rng.uniform(-1.0, 1.0, f.shape) * noise * np.abs(f).max()
        diag = neb_reference(pos, f.astype(np.float32), e.astype(np.float32), p["node_ptr"], case.band_ptr, p["cell"], p["pbc"], [spring] * B,
                             [1] * B)[4]
        pos, vel, st, bf, ft, seg, climber = neb_step_reference(pos, vel, f.astype(np.float32), e.astype(np.float32), p["node_ptr"], case.band_ptr,
                                                                p["cell"], p["pbc"], [spring] * B, [1] * B, st, fmax, dt_max=dt_max)
        log.append((e, climber.copy(), diag))
    return pos, st, climber, log


@functools.lru_cache(maxsize=None)
def neb_cgcnn_reference():
    return neb_reference_trajectory(neb_case(), **NEB_ARGS)


def test_oracle_cgcnn_bands_move_at_held_lists_and_noise_sensitivity():
    """20 band steps with dt = 3, dt_max = 30, fmax = 0, spring = 0.01 (an untrained model's forces are of order 1e-3 per A, its
    energies of order 1e-2: the spring is of the size of the curvature).  Measured here: largest displacement of an atom 0.62 A,
    the climber of each band the same image throughout and ahead of the runner-up by >= 1e-3 relative, DEV = 3.34e-5 A."""
    case = neb_case()
    pos, st, climber, log = neb_cgcnn_reference()
    assert (st["steps"] == NEB_ARGS["steps"]).all() and not st["done"].any()
    moved = np.sqrt(((pos - case.p["pos"]) ** 2).sum(1)).max()
    print("largest displacement %.3e A, climbers %s, energies at the start %s" % (moved, climber, log[0][0]))
    assert moved >= 0.05
    ends = np.zeros(len(pos), bool)
    for b in range(len(case.band_ptr) - 1):
        for s in (case.band_ptr[b], case.band_ptr[b + 1] - 1):
            ends[case.p["node_ptr"][s]:case.p["node_ptr"][s + 1]] = True
    assert np.array_equal(pos[ends], case.p["pos"][ends])
    for e, cl, diag in log:                                       # no decision of the trajectory depends on rounding
        assert np.array_equal(cl, climber)
        for b in range(len(case.band_ptr) - 1):
            inner = np.sort(e[case.band_ptr[b] + 1:case.band_ptr[b + 1] - 1])
            assert inner[-1] - inner[-2] >= 1e-3 * abs(inner[-1]), (b, inner)
        assert all(d["wrap"] >= 1e-3 for d in diag)
    gaps = min(g for _, _, diag in log for d in diag for g in d["gaps"][:3])
    print("smallest relative gap of two compared energies %.3e" % gaps)
    noisy = neb_reference_trajectory(case, noise=1e-4, seed=1, **NEB_ARGS)[0]
    dev = float(np.sqrt(((noisy - pos) ** 2).sum(1)).max())
    print("DEV = %.3e A (NEB_TRAJ_BOUND %.1e)" % (dev, NEB_TRAJ_BOUND))
    assert 0.0 < dev <= NEB_TRAJ_BOUND / 10
