"""GPU tests of the molecular pressure and of scaling by molecular centres of mass (include/emdee_hip.h:
emdee_md_molecular_pressure_tensor, emdee_md_set_molecular_scaling; csrc/settle.hpp) against the numpy yardstick of
tests/helpers/molecular_ref.py: constant pressure for the rigid molecules of tests/test_gpu_settle.py.

All boxes are settle_ref.water_box sized: 450 atoms (150 molecules of masses (16, 1, 1)) in a box of sides (7.0, 7.5, 8.2) at
lo = (-1.0, 0.5, 2.0), two cells per side, every atom wrapped on its own so that molecules straddle box and cell faces; one box
of 300 molecules with the same lattice spacing takes the molecular sums over two blocks.

Bounds.  Molecular sums: fp64 sums of per-molecule terms computed in fp64 from the engine's own state -- 1e-12 of the largest
component of K or W, in both precisions (a Float32 engine's reference is fed the engine's fp32 values: the absolute records
through pack_positions, which returns them as they are).  Against the all-pairs numpy sums: TOL[float64] of
tests/test_gpu_virial_tensor.py.  Positions, velocities, box lengths and scale factors of trajectories: the 1e-11 L_max and
1e-11 v_rms of tests/test_gpu_settle.py (lengths against L_max, factors, which are near 1, absolutely).  Forces against a fresh
engine: the 1e-12 (fp64) and 1e-4 (fp32) of tests/test_gpu_barostat.py."""
import ctypes as C

import numpy as np
import pytest

from .helpers import barostat_ref as bref
from .helpers import molecular_ref as mr
from .helpers import ortho_ref as oref
from .helpers import settle_ref as sr
from .test_gpu_dd_pairs import _build
from .test_gpu_settle import DT, EPS32, ERR_INVALID, ERR_STATE, _constraints_hold, _engine, _forces, _refused, _xv
from .test_gpu_virial_tensor import TOL as TENSOR_TOL
from .test_molecular_ref_host import FD_BOUND, H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

SUMS = 1e-12                                            # molecular sums against the engine-fed reference
X_TOL, V_TOL = 1e-11, 1e-11                             # tests/test_gpu_settle.py: _against_reference
FRESH = {np.float64: 1e-12, np.float32: 1e-4}           # tests/test_gpu_barostat.py: a scaled engine against a fresh one
MU = np.array([1.013, 0.991, 1.004])
# the Berendsen setting of the trajectories: p_ref 20 (12, 28) above the starting P_mol of -1.2, compressibilities near 0.02,
# tau_p = 1, every = 5 at dt = 0.002: every event shrinks a side by about 1e-3, and 7.0 stays far above 2 (rc + skin) = 5.8
P_REF, BETA, TAU_P, EVERY = np.array([19.0, 11.0, 27.0]), np.array([0.02, 0.025, 0.015]), 1.0, 5
# 300 molecules on the lattice spacing of the shared box: settle_ref.water_box puts n_mol on a side x side x (side + 1) lattice
BIG_N = 300
BIG_LENGTHS = sr.LENGTHS / np.array([6.0, 6.0, 7.0]) * np.array([7.0, 7.0, 8.0])


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _box_engine(E, dev, B, pos, vel, lengths, dtype=np.float64, masses=True, rigid=True, mol=None):
    """_engine of tests/test_gpu_settle.py for a box of other lengths (and a state of its own)"""
    im = E.cu((1.0 / B["mass"]).astype(dtype), dev) if masses else None
    lengths = [float(t) for t in lengths]
    md = E.VelocityVerlet(E.cu(np.asarray(pos).astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), lengths[0],
                          E.LennardJonesModel(sr.RC, sr.RS), E.cu(B["atoms"], dev), skin=sr.SKIN, inv_mass=im, lo=list(sr.LO),
                          lengths=lengths, periodic=[1, 1, 1])
    md.set_exclusions_(B["excl"])
    if rigid:
        mol = B["mol"] if mol is None else mol
        md.set_rigid3_(mol, B["geom"][:len(mol)])
    return md


def _image_gap(x, xr, lengths):
    d = np.asarray(x, dtype=np.float64) - xr
    return np.abs(d - lengths * np.rint(d / lengths)).max()


def _wrapped(x, lengths):
    return sr.LO + np.mod(x - sr.LO, lengths)


def _records(md, n):
    """the absolute records of an engine with masses, as they are (pack_positions with a zero shift)"""
    ids = torch.arange(n, dtype=torch.int32, device=md.device)
    return md.pack_positions(ids, [0.0, 0.0, 0.0]).cpu().numpy().astype(np.float64)


def _check_sums(md, B, mol, lengths, what, records=False, allpairs=None):
    """molecular_tensor_sums against molecular_ref fed the engine's own state, forces and tensor_sums; allpairs: keyword
    arguments of ortho_ref.total for the independent check"""
    x, v = _xv(md)
    if records:
        x = _records(md, x.shape[0])
    u = sr.unwrap(x, mol, lengths)
    f = _forces(md)
    atomic = np.array(md.tensor_sums())
    got = np.array(md.molecular_tensor_sums())
    assert np.array_equal(np.array(md.tensor_sums()), atomic)                 # (the query leaves the atomic sums as they are)
    cw, ck = mr.corrections(u, v, f, mol, B["mass"])
    want = atomic - np.concatenate([cw, ck])
    scale, err = np.abs(atomic).max(), np.abs(got - want).max()
    print("%s: max |sums - reference| = %.3e, largest component %.3e (bound %.0e relative); tr W_mol = %.4f, tr W = %.4f"
          % (what, err, scale, SUMS, got[:3].sum(), atomic[:3].sum()))
    assert err <= SUMS * scale, (what, err, scale)
    assert abs(got[:3].sum() - atomic[:3].sum()) > 1e-3 * abs(atomic[:3].sum())   # (the two formulations differ)
    if allpairs is not None:
        ref = oref.total(_wrapped(u, lengths), sr.LO, np.asarray(lengths), [1, 1, 1], sr.RC, sr.RS, B["atoms"], **allpairs)
        Wm, Km = mr.molecular_sums(u, v, ref["f"], ref["t"], mol, B["mass"])
        err = np.abs(got - np.concatenate([Wm, Km])).max()
        print("%s: against the all-pairs sums %.3e (bound %.0e relative)" % (what, err, TENSOR_TOL[np.float64]))
        assert err <= TENSOR_TOL[np.float64] * scale
    return got


# ---------------------------------------------------------------- 1. the molecular sums
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_molecular_sums_match_the_reference_before_and_after_steps(emdee, dev, dtype):
    B = sr.water_box()
    md = _engine(emdee, dev, B, dtype)
    name = np.dtype(dtype).name
    f32 = dtype == np.float32
    md.profile_(True)
    _check_sums(md, B, B["mol"], sr.LENGTHS, name + ", start", records=f32, allpairs=None if f32 else dict(excl=B["excl"]))
    ms, launches = md.kernel_time("molecular")
    assert launches == 1 and ms > 0.0                                        # (emdee_md_kernel_time index 10)
    assert md.kernel_time("settle")[1] == 0                                  # (index 9 stays the constraint stages)
    builds = md.nbr_stats()["builds"]
    md.step_(25, DT, 3)
    assert md.nbr_stats()["builds"] >= builds + 8                            # (slots are permuted)
    _check_sums(md, B, B["mol"], sr.LENGTHS, name + ", after 25 steps", records=f32)
    md.close()


def test_molecular_sums_over_two_blocks_of_molecules(emdee, dev):
    B = sr.water_box(n_mol=BIG_N, lengths=BIG_LENGTHS)
    assert B["mol"].shape[0] > 256                                           # (two blocks of RED_BLOCK molecules)
    md = _box_engine(emdee, dev, B, B["pos"], B["vel"], BIG_LENGTHS)
    _check_sums(md, B, B["mol"], BIG_LENGTHS, "300 molecules", allpairs=dict(excl=B["excl"]))
    md.close()


def test_atoms_outside_the_table_are_molecules_of_one(emdee, dev):
    B = sr.water_box()
    mol = B["mol"][:120]
    md = _box_engine(emdee, dev, B, B["pos"], B["vel"], sr.LENGTHS, mol=mol)
    got = _check_sums(md, B, mol, sr.LENGTHS, "120 of 150 molecules", allpairs=dict(excl=B["excl"]))
    full = _engine(emdee, dev, B)
    assert np.abs(got - np.array(full.molecular_tensor_sums())).max() > 1e-3 * np.abs(got).max()
    md.step_(5, DT)
    _check_sums(md, B, mol, sr.LENGTHS, "120 of 150 molecules, 5 steps")
    md.close()
    full.close()


def test_molecular_sums_of_a_charged_engine_under_ewald(emdee, dev):
    B = sr.water_box()
    md = _engine(emdee, dev, B, rigid=False)
    md.set_coulomb_(B["charges"], 1.0)
    md.set_ewald_(1.2, 6)
    md.set_rigid3_(B["mol"], B["geom"])
    _check_sums(md, B, B["mol"], sr.LENGTHS, "Ewald")
    md.step_(5, DT)
    _check_sums(md, B, B["mol"], sr.LENGTHS, "Ewald, 5 steps")
    md.close()


# ---------------------------------------------------------------- 2. without a table
def test_without_a_table_the_query_is_the_atomic_one_bit_for_bit(emdee, dev):
    B = sr.water_box()
    md = _engine(emdee, dev, B, rigid=False)
    assert md.molecular_tensor_sums() == md.tensor_sums()
    md.step_(7, DT)
    assert md.molecular_tensor_sums() == md.tensor_sums()
    P, Pm = md.pressure_tensor(), md.molecular_pressure_tensor()
    assert all(np.array_equal(P[k], Pm[k]) for k in P)
    md.close()


def test_without_a_table_the_switch_changes_nothing_bit_for_bit(emdee, dev):
    E = emdee
    B = sr.water_box()
    out = []
    for on in (False, True):
        md = _engine(E, dev, B, rigid=False)
        if on:
            md.set_molecular_scaling_()
        md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF[0], BETA[0], TAU_P, EVERY)
        md.step_(40, DT)
        out.append(_xv(md) + (np.array(md.box()[1]),))
        md.close()
    assert (out[0][2] < sr.LENGTHS).all()
    for a, b in zip(*out):
        assert np.array_equal(a, b)


# ---------------------------------------------------------------- 3. the scale primitive
@pytest.mark.parametrize("case", ["f64", "f32", "f32-cell-relative"])
def test_molecular_scale_translates_molecules_and_keeps_their_geometry(emdee, dev, case):
    E = emdee
    dtype = np.float64 if case == "f64" else np.float32
    masses = case != "f32-cell-relative"
    B = sr.water_box()
    if not masses:                                                           # (tests/test_gpu_settle.py: the cell-relative case)
        B["mass"] = np.ones_like(B["mass"])
        B["vel"] = sr.rattle(B["unwrapped"], B["vel"], B["mol"], B["mass"])
    md = _engine(E, dev, B, dtype, masses=masses)
    md.set_molecular_scaling_()
    md.profile_(True)
    x0, v0 = _xv(md)
    v0_raw = md.state(forces=False)["velocities"].cpu().numpy()
    builds = md.nbr_stats()["builds"]
    md.scale_box_(MU)
    assert md.kernel_time("molecular")[1] == 1
    ln = np.array(md.box()[1])
    assert np.array_equal(ln, MU * sr.LENGTHS) and md.box()[0] == list(sr.LO)
    assert md.nbr_stats()["builds"] > builds
    x1, v1 = _xv(md)
    assert np.array_equal(md.state(forces=False)["velocities"].cpu().numpy(), v0_raw)     # velocity_scale = 1: bit for bit
    xr, vr, lr = mr.scale(sr.unwrap(x0, B["mol"], sr.LENGTHS), v0, sr.LO, sr.LENGTHS, MU, B["mol"], B["mass"])
    gap = _image_gap(x1, xr, ln)
    if dtype == np.float64:
        bound = X_TOL * sr.LENGTHS.max()
    else:
        # x0 as read is rounded once by get_state, the new record once, and get_state rounds again: 3 half ulp_fp32 of the largest
        # coordinate, bound 2 ulp
        bound = 2.0 * float(np.spacing(np.float32(np.abs(x1).max())))
    print("%s: positions against the reference modulo the new box %.3e (bound %.3e)" % (case, gap, bound))
    assert gap <= bound
    assert sr.residual(sr.unwrap(x1, B["mol"], ln), B["mol"], B["geom"]) <= (1e-12 if dtype == np.float64 else
                                                                            8.0 * float(np.spacing(np.float32(np.abs(x1).max()))) / sr.D_LEG)
    # forces: those of a fresh engine loaded with the scaled state
    fresh = _box_engine(E, dev, B, x1, v1, ln, dtype, masses=masses)
    f, ff = _forces(md), _forces(fresh)
    print("%s: forces against a fresh engine %.3e of %.3e" % (case, np.abs(f - ff).max(), np.abs(ff).max()))
    assert np.abs(f - ff).max() <= FRESH[dtype] * np.abs(ff).max()
    fresh.close()
    # and back
    md.scale_box_(1.0 / MU)
    back = np.array(md.box()[1])
    assert np.abs(back - sr.LENGTHS).max() <= 4e-16 * sr.LENGTHS.max()       # (mu x 1 / mu: an ulp)
    x2, _ = _xv(md)
    gap = _image_gap(x2, x0, back)
    print("%s: positions after the scale back %.3e" % (case, gap))
    assert gap <= (X_TOL * sr.LENGTHS.max() if dtype == np.float64 else 2.0 * bound)
    if masses:
        _constraints_hold(md, B, dtype, case + ", scaled there and back", records=dtype == np.float32)
    else:
        # the bounds of tests/test_gpu_settle.py: test_constraints_hold_on_cell_relative_float32_records (caller-order positions)
        x, v = _xv(md)
        u = sr.unwrap(x, B["mol"], sr.LENGTHS)
        ulp = float(np.spacing(np.float32(np.abs(x).max())))
        res, left = sr.residual(u, B["mol"], B["geom"]), sr.bond_velocities(u, v, B["mol"]).max()
        tol_x, tol_v = 8.0 * ulp / sr.D_LEG, 8.0 * EPS32 + 2.0 * np.sqrt(3.0) * ulp / sr.D_LEG
        print("%s: distance error %.3e (bound %.3e), bond-relative velocity %.3e (bound %.3e)" % (case, res, tol_x, left, tol_v))
        assert res <= tol_x and left <= tol_v
    md.step_(3, DT)                                                          # the engine steps on
    md.close()


def test_velocity_scale_acts_on_the_centres_of_mass_alone(emdee, dev):
    B = sr.water_box()
    md = _engine(emdee, dev, B)
    md.set_molecular_scaling_()
    x0, v0 = _xv(md)
    md.scale_box_(1.0, 0.5)
    x1, v1 = _xv(md)
    assert md.box()[1] == list(sr.LENGTHS)
    assert np.abs(x1 - x0).max() <= 1e-14 * np.abs(x0).max()
    u = sr.unwrap(x0, B["mol"], sr.LENGTHS)
    _, V0, _, _ = mr.centres(u, v0, B["mol"], B["mass"])
    _, V1, _, _ = mr.centres(u, v1, B["mol"], B["mass"])
    vmax = np.abs(v0).max()
    assert np.abs(V1 - 0.5 * V0).max() <= 1e-14 * vmax
    assert np.abs((v1[B["mol"]] - V1[:, None]) - (v0[B["mol"]] - V0[:, None])).max() <= 1e-14 * vmax
    assert np.abs(V0).max() > 0.05 * vmax                                    # (there was something to halve)
    _constraints_hold(md, B, np.float64, "velocity_scale = 0.5")
    md.close()


def test_molecular_scale_of_a_partial_table_scales_the_other_atoms_one_by_one(emdee, dev):
    B = sr.water_box()
    mol = B["mol"][:120]
    md = _box_engine(emdee, dev, B, B["pos"], B["vel"], sr.LENGTHS, mol=mol)
    md.set_molecular_scaling_()
    x0, v0 = _xv(md)
    md.scale_box_(MU, 0.5)
    x1, v1 = _xv(md)
    ln = np.array(md.box()[1])
    xr, vr, _ = mr.scale(sr.unwrap(x0, mol, sr.LENGTHS), v0, sr.LO, sr.LENGTHS, MU, mol, B["mass"], 0.5)
    assert _image_gap(x1, xr, ln) <= X_TOL * sr.LENGTHS.max()
    assert np.abs(v1 - vr).max() <= 1e-14 * np.abs(v0).max()
    assert np.array_equal(v1[360:], 0.5 * v0[360:])                          # (the atom-by-atom kernel's own arithmetic)
    md.close()


# ---------------------------------------------------------------- 4. the finite difference on the device
def test_trace_of_the_molecular_virial_is_the_engines_own_volume_derivative(emdee, dev):
    B = sr.water_box()
    md = _engine(emdee, dev, B)
    md.set_molecular_scaling_()
    trace = sum(md.molecular_tensor_sums()[:3])
    md.scale_box_(1.0 + H)
    up = md.totals()[0]
    md.scale_box_((1.0 - H) / (1.0 + H))                                     # (molecular scales compose: this is mu = 1 - h of the start)
    assert np.abs(np.array(md.box()[1]) / sr.LENGTHS - (1.0 - H)).max() <= 1e-15
    down = md.totals()[0]
    fd = -(up - down) / (2.0 * H)
    gap = abs(fd - trace) / abs(trace)
    print("tr W_mol = %.4f, -dU/dmu through scale_box_ and totals() = %.4f: relative difference %.3e (bound %.2e)" % (trace, fd, gap, FD_BOUND))
    assert gap <= FD_BOUND
    md.close()


# ---------------------------------------------------------------- 5. trajectories
def _coupled_against_reference(E, dev, B, kind, coupling, nsteps, what, langevin=None, crescale=None):
    """the engine, one step per call, against molecular_ref.coupled_constrained_verlet.  The reference takes the engine's
    forces after every step, as tests/test_gpu_settle.py: _against_reference does; the step of an event needs the forces and the
    atomic virial sums BEFORE the event, which the engine has left behind by then: a second engine (no table, no coupling)
    loaded with the reference's positions on the reference's box evaluates them with the same kernels."""
    md = _engine(E, dev, B)
    md.set_molecular_scaling_()
    names = {bref.ISOTROPIC: "isotropic", bref.SEMIISOTROPIC: "semiisotropic", bref.ANISOTROPIC: "anisotropic"}
    if kind == bref.BERENDSEN:
        md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF, BETA, TAU_P, EVERY, coupling=names[coupling])
    else:
        md.set_barostat_(E.BAROSTAT_CRESCALE, P_REF[0], BETA[0], TAU_P, EVERY, temperature=crescale[0], seed=crescale[1])
    lv = None
    if langevin is not None:
        gamma, temp, seed = langevin
        md.set_langevin_(gamma, temp, seed=seed)
        ids = torch.arange(B["pos"].shape[0])
        lv = (gamma, temp, lambda k: md.langevin_normals(seed, k, ids).cpu().numpy())
    x_start = B["unwrapped"]
    offset = B["pos"] - B["unwrapped"]
    held, boxes, seen = {}, {0: np.array(md.box()[1])}, {}

    def force(x, ln, k):
        if k <= 0:
            return _forces(md)
        md.step_(1, DT)
        boxes[k] = np.array(md.box()[1])
        if k % EVERY:
            return _forces(md)
        twin = _box_engine(E, dev, B, _wrapped(x, ln), np.zeros_like(x), ln, rigid=False)
        held[k] = np.array(twin.tensor_sums()[:6])
        f = _forces(twin)
        twin.close()
        return f

    def observe(s, x, v, ln):
        gx, gv = _xv(md)
        # offset: whole lengths of the starting box, which the scales turned into whole lengths of the present one
        whole = np.rint(offset / sr.LENGTHS) * ln
        seen[s] = (np.abs(gx - (x + whole)).max(), np.abs(gv - v).max(), np.sqrt((v * v).sum(axis=1).mean()), np.abs(boxes[s] - ln).max())

    xi = None if crescale is None else (lambda count: float(md.langevin_normals(crescale[1], count, torch.tensor([-1]))[0, 0]))
    x, v, ln, events = mr.coupled_constrained_verlet(x_start, B["vel"], force, lambda x, ln, s: held[s], nsteps, DT, B["mol"], B["geom"], B["mass"],
                                                     sr.LO, sr.LENGTHS, kind, P_REF, BETA, TAU_P, EVERY, coupling,
                                                     temperature=None if crescale is None else crescale[0], xi=xi, langevin=lv, observe=observe)
    assert len(events) == nsteps // EVERY
    for s, P, mu, vs in events:
        got = boxes[s] / boxes[s - 1]
        print("%s, event at step %d: P_mol = %s, mu = %s, engine's mu off by %.3e" % (what, s, P, mu, np.abs(got - mu).max()))
        assert (np.abs(mu - 1.0) > 1e-6).all()                               # (the scale is exercised)
        assert np.abs(got - mu).max() <= X_TOL
    for s in sorted(seen):
        ex, ev, vrms, el = seen[s]
        if s in (1, EVERY, nsteps):
            print("%s, step %d: max |dx| = %.3e, max |dv| = %.3e (rms velocity %.3f), box %.3e" % (what, s, ex, ev, vrms, el))
        assert ex <= X_TOL * sr.LENGTHS.max() and ev <= V_TOL * vrms and el <= X_TOL * sr.LENGTHS.max(), (what, s, ex, ev, el)
    _constraints_hold_on(md, B, ln, what)
    return md


def _constraints_hold_on(md, B, lengths, what):
    """_constraints_hold of tests/test_gpu_settle.py (fp64 bounds) on a box of other lengths"""
    x, v = _xv(md)
    u = sr.unwrap(x, B["mol"], lengths)
    res, left = sr.residual(u, B["mol"], B["geom"]), sr.bond_velocities(u, v, B["mol"]).max()
    print("%s: largest relative distance error %.3e, largest bond-relative velocity / (|v| d) %.3e (bounds 1e-12)" % (what, res, left))
    assert res <= 1e-12 and left <= 1e-12, (what, res, left)


@pytest.mark.parametrize("coupling", ["isotropic", "semiisotropic", "anisotropic"])
def test_berendsen_trajectory_of_rigid_molecules_matches_the_reference(emdee, dev, coupling):
    B = sr.water_box()
    c = {"isotropic": bref.ISOTROPIC, "semiisotropic": bref.SEMIISOTROPIC, "anisotropic": bref.ANISOTROPIC}[coupling]
    md = _coupled_against_reference(emdee, dev, B, bref.BERENDSEN, c, 20, "Berendsen " + coupling)
    ln = np.array(md.box()[1])
    if coupling == "isotropic":
        assert np.abs(ln / sr.LENGTHS - ln[0] / sr.LENGTHS[0]).max() <= 4e-15   # (one factor; four roundings per side)
    if coupling == "semiisotropic":
        assert abs(ln[0] / sr.LENGTHS[0] - ln[1] / sr.LENGTHS[1]) <= 4e-15 < abs(ln[0] / sr.LENGTHS[0] - ln[2] / sr.LENGTHS[2])
    if coupling == "anisotropic":
        assert len(set(np.round(ln / sr.LENGTHS, 9))) == 3
    md.close()


def test_crescale_with_langevin_matches_the_reference_and_is_reproducible(emdee, dev):
    E = emdee
    B = sr.water_box()
    seed, T = 12345, 1.0
    md = _coupled_against_reference(E, dev, B, bref.CRESCALE, bref.ISOTROPIC, 20, "C-rescale with Langevin", langevin=(1.0, T, 7),
                                    crescale=(T, seed))
    md.close()
    out = []
    for sd in (seed, seed, seed + 1):
        md = _engine(E, dev, B)
        md.set_molecular_scaling_()
        md.set_langevin_(1.0, T, seed=7)
        md.set_barostat_(E.BAROSTAT_CRESCALE, P_REF[0], BETA[0], TAU_P, EVERY, temperature=T, seed=sd)
        md.step_(20, DT)
        out.append(_xv(md) + (np.array(md.box()[1]),))
        md.close()
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    assert not np.array_equal(out[0][2], out[2][2])


# ---------------------------------------------------------------- 6. batching
@pytest.mark.parametrize("rebuild_every", [0, 3])
def test_the_states_of_a_rigid_coupled_engine_do_not_depend_on_the_dealing(emdee, dev, rebuild_every):
    E = emdee
    B = sr.water_box()
    out = []
    for deal in ((40,), (5,) * 8, (1,) * 40):
        md = _engine(E, dev, B)
        md.set_molecular_scaling_()
        md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF[0], BETA[0], TAU_P, EVERY)
        md.profile_(True)
        for n in deal:
            md.step_(n, DT, rebuild_every)
        assert md.kernel_time("settle")[1] == 3 * 40                         # (index 9 stays the constraint stages)
        assert md.kernel_time("molecular")[1] == 2 * (40 // EVERY)           # (one sum and one scale per event)
        out.append(_xv(md) + (np.array(md.box()[1]),))
        md.close()
    assert (out[0][2] < sr.LENGTHS).all()
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert np.array_equal(a, b)


# ---------------------------------------------------------------- 7. the switch and the refusals
def test_switch_on_lifts_the_three_refusals_and_off_is_refused_while_coupled(emdee, dev):
    E = emdee
    B = sr.water_box()
    md = _engine(E, dev, B)
    _refused(E, ERR_STATE, md.scale_box_, 1.001)                             # (the default: as before)
    _refused(E, ERR_INVALID, E._lib.call, "emdee_md_set_molecular_scaling", md._handle, 2)
    _refused(E, ERR_INVALID, E._lib.call, "emdee_md_set_molecular_scaling", md._handle, -1)
    _refused(E, ERR_STATE, md.scale_box_, 1.001)                             # (a refused call changes nothing)
    md.set_molecular_scaling_()
    md.scale_box_(1.001)
    md.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF[0], BETA[0], TAU_P, EVERY)
    text = _refused(E, ERR_STATE, md.set_molecular_scaling_, False)
    assert "coupling" in text
    before = md.box()[1]
    md.step_(EVERY, DT)                                                      # the setting stayed: still coupled
    assert md.box()[1] != before
    _constraints_hold_on(md, B, np.array(md.box()[1]), "coupled after the refused switch-off")
    md.set_barostat_(None)
    md.set_molecular_scaling_(False)
    _refused(E, ERR_STATE, md.scale_box_, 1.001)
    _refused(E, ERR_STATE, md.set_barostat_, E.BAROSTAT_BERENDSEN, 1.0, 0.01, 1.0, 5)
    md.close()
    # a barostat first, the table second
    other = _engine(E, dev, B, rigid=False)
    other.set_barostat_(E.BAROSTAT_BERENDSEN, P_REF[0], BETA[0], TAU_P, EVERY)
    _refused(E, ERR_STATE, other.set_rigid3_, B["mol"], B["geom"])
    other.set_molecular_scaling_()
    other.set_rigid3_(B["mol"], B["geom"])
    other.step_(EVERY, DT)
    assert other.box()[1] != list(sr.LENGTHS)
    other.set_rigid3_(None, None)                                            # no table: the switch may go off under a barostat
    other.set_molecular_scaling_(False)
    other.close()


def test_a_lent_engine_refuses_the_switch(emdee, dev):
    E = emdee
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    text = _refused(E, ERR_STATE, dd.engine(0).set_molecular_scaling_)
    assert "emdee_dd_engine" in text
    dd.step_(2, 0.005)
    dd.close()


def test_a_stale_table_refuses_the_scale_and_the_query(emdee, dev):
    E = emdee
    B = sr.water_box()
    ghostly = B["atoms"].copy()
    ghostly["twice_sqrt_eps"] = 0.0                                          # (tests/test_gpu_settle.py: the rules of the table alone)
    md = _engine(E, dev, B, excl=False, atoms=ghostly)
    md.set_molecular_scaling_()
    md.set_state_(E.cu(B["pos"][:447], dev), E.cu(B["vel"][:447], dev), E.cu(ghostly[:447], dev), E.cu(1.0 / B["mass"][:447], dev))
    _refused(E, ERR_STATE, md.scale_box_, 1.001)
    _refused(E, ERR_STATE, md.molecular_tensor_sums)
    assert md.box()[1] == list(sr.LENGTHS)
    md.tensor_sums()                                                         # (the atomic query does not look at the table)
    md.set_rigid3_(None, None)
    md.scale_box_(1.001)
    assert md.molecular_tensor_sums() == md.tensor_sums()
    md.close()
    # before emdee_md_set_state, through the C ABI
    ctx = E.context_for(dev)
    h = C.c_void_p()
    three = lambda *v: (C.c_double * 3)(*v)
    E._lib.call("emdee_md_create", ctx.handle, three(*sr.LO), three(*sr.LENGTHS), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(E.LennardJonesModel(sr.RC, sr.RS)), sr.SKIN, 8, C.byref(h))
    _refused(E, ERR_STATE, E._lib.call, "emdee_md_molecular_pressure_tensor", h, (C.c_double * 12)())
    _refused(E, ERR_INVALID, E._lib.call, "emdee_md_molecular_pressure_tensor", h, None)
    E._lib.call("emdee_md_set_molecular_scaling", h, 1)
    E._lib.call("emdee_md_destroy", h)


def test_a_scale_refused_at_an_event_comes_back_from_step_with_the_constraints_holding(emdee, dev):
    """A compressibility of 1.5 asks the first event for mu near 0.7: the box would fall below 2 (rc + skin) = 5.8.  The step call
    returns EMDEE_ERR_STATE, the box is untouched and the state is the completed step's, rigid as ever."""
    E = emdee
    B = sr.water_box()
    md = _engine(E, dev, B)
    md.set_molecular_scaling_()
    md.set_barostat_(E.BAROSTAT_BERENDSEN, 100.0, 1.5, 1.0, 3)
    text = _refused(E, ERR_STATE, md.step_, 10, DT)
    assert "coupling" in text
    assert md.box()[1] == list(sr.LENGTHS)
    twin = _engine(E, dev, B)
    twin.step_(3, DT)
    for a, b in zip(_xv(md), _xv(twin)):
        assert np.abs(a - b).max() <= 1e-12
    _constraints_hold(md, B, np.float64, "after the refused event")
    md.set_barostat_(None)
    md.step_(2, DT)                                                          # still able to step
    md.close()
    twin.close()
