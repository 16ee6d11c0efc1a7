"""GPU tests of rigid three-site molecules (include/emdee_hip.h: emdee_md_set_rigid3; csrc/settle.hpp) against the numpy
yardstick of tests/helpers/settle_ref.py: iterative SHAKE and RATTLE around a force callback, no SETTLE formulas.

One small box for all of them (settle_ref.water_box): 150 molecules of masses (16, 1, 1) with d_leg = 0.32 and d_base = 0.50 in a
box of sides (7.0, 7.5, 8.2) at lo = (-1.0, 0.5, 2.0), rc = 2.5, skin = 0.4 (two cells per side), half_sigma 0.5 on the centre
and 0.2 on the legs, intramolecular pairs excluded, centres on a jittered lattice, random orientations, every atom wrapped on its
own so that molecules straddle box faces and cell faces, velocities projected by the reference, dt = 0.002."""
import numpy as np
import pytest

from .helpers import settle_ref as sr
from .test_gpu_dd_pairs import _build

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
DT = sr.DT
EPS32 = float(np.finfo(np.float32).eps)
# max |E(t) - E(0)| of the numpy reference (constrained_verlet with the all-pairs forces of tests/helpers/ortho_ref.py) from the
# same start over 400 steps, sampled every 20; E(0) = -220.362405.  Measured on the CPU, 2026-10-18:
#   python -m tests.helpers.settle_ref
REFERENCE_DRIFT = 1.246042e-03


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _engine(E, dev, B, dtype=np.float64, masses=True, excl=True, rigid=True, vel=None, atoms=None):
    im = E.cu((1.0 / B["mass"]).astype(dtype), dev) if masses else None
    vel = B["vel"] if vel is None else vel
    md = E.VelocityVerlet(E.cu(B["pos"].astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), float(sr.LENGTHS[0]),
                          E.LennardJonesModel(sr.RC, sr.RS), E.cu(B["atoms"] if atoms is None else atoms, dev), skin=sr.SKIN, inv_mass=im,
                          lo=list(sr.LO), lengths=list(sr.LENGTHS), periodic=[1, 1, 1])
    if excl:
        md.set_exclusions_(B["excl"])
    if rigid:
        md.set_rigid3_(B["mol"], B["geom"])
    return md


def _xv(md):
    st = md.state(forces=False)
    return st["positions"].cpu().numpy().astype(np.float64), st["velocities"].cpu().numpy().astype(np.float64)


def _forces(md):
    return md.state(positions=False, velocities=False)["forces"].cpu().numpy().astype(np.float64)


def _refused(E, code, call, *args, **kw):
    with pytest.raises(E.EmDeeError) as err:
        call(*args, **kw)
    assert err.value.code == code, str(err.value)
    return str(err.value)


def _against_reference(md, x_start, v_start, offset, B, checkpoints, rebuild_every, what):
    """the engine, one step per call, against constrained_verlet fed the engine's own forces; x_start unwrapped, offset = what
    the engine's caller-order positions differ from it by (whole box lengths)"""
    seen = {}

    def force(x, k):
        if k > 0:
            md.step_(1, DT, rebuild_every)
        return _forces(md)

    def observe(s, x, v):
        if s in checkpoints:
            gx, gv = _xv(md)
            seen[s] = (np.abs(gx - (x + offset)).max(), np.abs(gv - v).max(), np.sqrt((v * v).sum(axis=1).mean()))
    sr.constrained_verlet(x_start, v_start, force, max(checkpoints), DT, B["mol"], B["geom"], B["mass"], observe=observe)
    for s in checkpoints:
        ex, ev, vrms = seen[s]
        print("%s, step %d: max |dx| = %.3e (box side %.1f), max |dv| = %.3e (rms velocity %.3f)" % (what, s, ex, sr.LENGTHS.max(), ev, vrms))
        assert ex <= 1e-11 * sr.LENGTHS.max() and ev <= 1e-11 * vrms, (what, s, ex, ev)


def _constraints_hold(md, B, dtype, what, records=False):
    """every distance and every bond-relative velocity of the engine's state within the bounds of the module docstring"""
    x, v = _xv(md)
    u = sr.unwrap(x, B["mol"], sr.LENGTHS)
    res = sr.residual(u, B["mol"], B["geom"])
    if dtype == np.float64:
        tol_x, tol_v = 1e-12, 1e-12
    else:
        # the rounding of the caller-order positions get_state returns (not of the records): 8 ulp_fp32(L_max) / d_leg
        tol_x = 8.0 * float(np.spacing(np.float32(np.abs(x).max()))) / sr.D_LEG
        tol_v = 8.0 * EPS32
    if records:
        # Float32 with masses keeps absolute records: pack_positions with a zero shift returns them as they are, the geometry
        # stage (e) itself used, without the rounding of record + box lengths in get_state
        ids = torch.arange(x.shape[0], dtype=torch.int32, device=md.device)
        u = sr.unwrap(md.pack_positions(ids, [0.0, 0.0, 0.0]).cpu().numpy().astype(np.float64), B["mol"], sr.LENGTHS)
    left = sr.bond_velocities(u, v, B["mol"]).max()
    print("%s: largest relative distance error %.3e (bound %.3e), largest bond-relative velocity / (|v| d) %.3e (bound %.3e)"
          % (what, res, tol_x, left, tol_v))
    assert res <= tol_x and left <= tol_v, (what, res, left)


# ---------------------------------------------------------------- 1. against the reference
def test_one_step_and_twenty_steps_match_the_reference(emdee, dev):
    B = sr.water_box()
    md = _engine(emdee, dev, B)
    _against_reference(md, B["unwrapped"], B["vel"], B["pos"] - B["unwrapped"], B, (1, 20), 3, "fp64, rebuild_every = 3")
    assert md.nbr_stats()["builds"] >= 1 + 20 // 3                           # (re-sorts fell between the two stages)
    md.close()


# ---------------------------------------------------------------- 2. the constraints hold
@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_constraints_hold_over_300_steps_with_automatic_rebuilds(emdee, dev, dtype, langevin):
    B = sr.water_box()
    md = _engine(emdee, dev, B, dtype)
    if langevin:
        md.set_langevin_(1.0, 1.0, seed=7)
    before = md.nbr_stats()["builds"]
    md.step_(300, DT)
    assert md.nbr_stats()["builds"] > before
    _constraints_hold(md, B, dtype, "%s, %s" % (np.dtype(dtype).name, "Langevin" if langevin else "NVE"), records=dtype == np.float32)
    md.close()


def test_constraints_hold_on_cell_relative_float32_records(emdee, dev):
    # Float32 without masses keeps cell-relative records (kernels.hpp RelGrid): the stages add the cells' origins in double.  All
    # masses 1.  The distance bound is that of the test above.  The velocity check reads caller-order positions here (the
    # records are relative), each off by up to ulp_fp32(L_max) / 2 per axis: a bond vector off by sqrt(3) ulp in length against a
    # relative velocity of up to 2 |v| adds 2 sqrt(3) ulp_fp32(L_max) / d to the 8 eps_fp32 of the records' own bound.
    B = sr.water_box()
    B["mass"] = np.ones_like(B["mass"])
    B["vel"] = sr.rattle(B["unwrapped"], B["vel"], B["mol"], B["mass"])
    md = _engine(emdee, dev, B, np.float32, masses=False)
    before = md.nbr_stats()["builds"]
    md.step_(300, DT)
    assert md.nbr_stats()["builds"] > before
    x, v = _xv(md)
    u = sr.unwrap(x, B["mol"], sr.LENGTHS)
    ulp = float(np.spacing(np.float32(np.abs(x).max())))
    res, left = sr.residual(u, B["mol"], B["geom"]), sr.bond_velocities(u, v, B["mol"]).max()
    tol_x, tol_v = 8.0 * ulp / sr.D_LEG, 8.0 * EPS32 + 2.0 * np.sqrt(3.0) * ulp / sr.D_LEG
    print("f32 cell-relative: distance error %.3e (bound %.3e), bond-relative velocity %.3e (bound %.3e)" % (res, tol_x, left, tol_v))
    assert res <= tol_x and left <= tol_v
    md.close()


# ---------------------------------------------------------------- 3. energy conservation
def test_energy_is_conserved_as_well_as_by_the_reference(emdee, dev):
    B = sr.water_box()
    md = _engine(emdee, dev, B)
    ep, ek, _ = md.totals()
    e0, worst = ep + ek, 0.0
    for _ in range(20):
        md.step_(20, DT)
        ep, ek, _ = md.totals()
        worst = max(worst, abs(ep + ek - e0))
    print("engine: E(0) = %.6f, max |E(t) - E(0)| over 400 steps = %.6e; reference %.6e" % (e0, worst, REFERENCE_DRIFT))
    assert abs(e0 - (-220.362405)) <= 1e-5                                   # (the same start as the reference's)
    assert worst <= 2.0 * REFERENCE_DRIFT                                    # (the factor: another summation order over 400 chaotic steps)
    md.close()


# ---------------------------------------------------------------- 4. dealing and reproducibility
def test_dealing_of_steps_to_calls_and_reruns_are_bit_identical(emdee, dev):
    B = sr.water_box()
    out = []
    for deal in ((40,), (5,) * 8, (1,) * 40, (40,)):
        md = _engine(emdee, dev, B)
        md.profile_(True)
        for n in deal:
            md.step_(n, DT)
        out.append(_xv(md))
        ms, launches = md.kernel_time("settle")
        assert launches == 3 * 40 and ms > 0.0                               # (stages (a), (c), (e) of every step; emdee_md_kernel_time index 9)
        md.close()
    for x, v in out[1:]:
        assert np.array_equal(x, out[0][0]) and np.array_equal(v, out[0][1])


# ---------------------------------------------------------------- 5. charged engines
def test_charged_engine_with_reaction_field_then_pme(emdee, dev):
    B = sr.water_box()
    md = _engine(emdee, dev, B, rigid=False)
    md.set_coulomb_(B["charges"], 1.0)
    md.set_rigid3_(B["mol"], B["geom"])
    _against_reference(md, B["unwrapped"], B["vel"], B["pos"] - B["unwrapped"], B, (1,), 0, "reaction field")
    md.step_(49, DT)
    _constraints_hold(md, B, np.float64, "reaction field, 50 steps")
    md.set_pme_(1.2, 16, 4)
    x, v = _xv(md)
    u = sr.unwrap(x, B["mol"], sr.LENGTHS)
    _against_reference(md, u, v, x - u, B, (1,), 0, "PME")
    md.step_(49, DT)
    _constraints_hold(md, B, np.float64, "PME, 50 steps")
    md.close()


# ---------------------------------------------------------------- 6. refusals and state rules
def test_invalid_tables_are_refused_and_the_previous_table_still_steps(emdee, dev):
    E = emdee
    B = sr.water_box()
    md = _engine(E, dev, B)
    mol, geom, n = B["mol"], B["geom"], B["mol"].shape[0]

    def changed(arr, m, k, value):
        out = arr.astype(np.float64 if arr is geom else np.int64).copy()
        out[m, k] = value
        return out
    one = torch.zeros(3, dtype=torch.int32, device=dev)
    cases = {
        "NULL atoms": lambda: E._lib.call("emdee_md_set_rigid3", md._handle, None, None, 1),
        "NULL geom": lambda: E._lib.call("emdee_md_set_rigid3", md._handle, one.data_ptr(), None, 1),
        "negative count": lambda: E._lib.call("emdee_md_set_rigid3", md._handle, one.data_ptr(), one.data_ptr(), -1),
        "id too high": lambda: md.set_rigid3_(changed(mol, 3, 1, 3 * n), geom),
        "negative id": lambda: md.set_rigid3_(changed(mol, 3, 0, -1), geom),
        "twice within": lambda: md.set_rigid3_(changed(mol, 4, 2, mol[4, 0]), geom),
        "twice across": lambda: md.set_rigid3_(changed(mol, 4, 2, mol[9, 1]), geom),
        "nan distance": lambda: md.set_rigid3_(mol, changed(geom, 2, 0, np.nan)),
        "infinite distance": lambda: md.set_rigid3_(mol, changed(geom, 2, 1, np.inf)),
        "zero distance": lambda: md.set_rigid3_(mol, changed(geom, 2, 1, 0.0)),
        "negative distance": lambda: md.set_rigid3_(mol, changed(geom, 2, 0, -0.32)),
        "no triangle": lambda: md.set_rigid3_(mol, changed(geom, 2, 1, 0.64)),
    }
    for name, call in cases.items():
        _refused(E, ERR_INVALID, call)
        md.step_(1, DT)
    # the device check: legs of different masses (the apex and a leg swapped), a distance 3 % off
    swapped = mol.copy()
    swapped[7] = mol[7, [1, 0, 2]]
    text = _refused(E, ERR_STATE, md.set_rigid3_, swapped, geom)
    assert "molecule 7 " in text and "masses" in text
    md.step_(1, DT)
    text = _refused(E, ERR_STATE, md.set_rigid3_, mol, changed(geom, 5, 0, 0.33))
    assert "molecule 5 " in text and "distance" in text
    md.step_(1, DT)
    # pressure coupling and rigid molecules exclude each other
    _refused(E, ERR_STATE, md.scale_box_, 1.001)
    _refused(E, ERR_STATE, md.set_barostat_, E.BAROSTAT_BERENDSEN, 1.0, 0.01, 1.0, 5)
    md.set_barostat_(E.BAROSTAT_OFF)
    md.step_(1, DT)
    _constraints_hold(md, B, np.float64, "after %d refusals" % (len(cases) + 4))       # (the table set at the start is the one in force)
    md.close()
    other = _engine(E, dev, B, rigid=False)
    other.set_barostat_(E.BAROSTAT_BERENDSEN, 1.0, 0.01, 1.0, 5)
    _refused(E, ERR_STATE, other.set_rigid3_, mol, geom)
    other.set_barostat_(E.BAROSTAT_OFF)
    other.set_rigid3_(mol, geom)
    other.step_(2, DT)
    other.close()


def test_an_engine_lent_by_a_decomposition_refuses_the_call(emdee, dev):
    E = emdee
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (two bricks of rc + skin + halo)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    text = _refused(E, ERR_STATE, dd.engine(0).set_rigid3_, [[0, 1, 2]], [[1.0, 1.5]])
    assert "emdee_dd_engine" in text
    dd.step_(2, 0.005)                                                                   # the decomposition is unharmed
    dd.close()


def test_clearing_the_table_restores_the_unconstrained_trajectory(emdee, dev):
    # The intramolecular pairs are excluded and nothing else holds a molecule together: 20 unconstrained steps are harmless.
    # Installing the table projects the velocities, so the twin that never had one starts from the state the install left.
    B = sr.water_box()
    md = _engine(emdee, dev, B)
    x, v = _xv(md)
    assert np.array_equal(x, B["pos"])                                       # (the call moved no atom)
    md.set_rigid3_(None, None)
    twin = _engine(emdee, dev, B, rigid=False, vel=v)
    md.step_(20, DT)
    twin.step_(20, DT)
    (xa, va), (xb, vb) = _xv(md), _xv(twin)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert sr.residual(sr.unwrap(xa, B["mol"], sr.LENGTHS), B["mol"], B["geom"]) > 1e-6        # (and it is unconstrained)
    md.close()
    twin.close()


def test_set_state_keeps_the_table_for_the_same_count_and_refuses_to_step_for_another(emdee, dev):
    # without exclusions (they would refuse the smaller state themselves) and without LJ forces (twice_sqrt_eps = 0): the rules
    # of the table alone
    E = emdee
    B = sr.water_box()
    ghostly = B["atoms"].copy()
    ghostly["twice_sqrt_eps"] = 0.0
    md = _engine(E, dev, B, excl=False, atoms=ghostly)
    rng = np.random.default_rng(3)
    raw = rng.normal(size=B["vel"].shape)                                    # velocities with bond components
    load = lambda n, vel: md.set_state_(E.cu(B["pos"][:n], dev), E.cu(vel[:n], dev), E.cu(ghostly[:n], dev), E.cu(1.0 / B["mass"][:n], dev))
    load(450, raw)
    x, v = _xv(md)
    assert sr.bond_velocities(sr.unwrap(x, B["mol"], sr.LENGTHS), v, B["mol"]).max() <= 1e-12      # (checked and projected again)
    assert np.abs(v - sr.rattle(B["unwrapped"], raw, B["mol"], B["mass"])).max() <= 1e-12 * np.abs(raw).max()
    md.step_(5, DT)
    _constraints_hold(md, B, np.float64, "after set_state with the same count")
    # the same count, a state that does not fit the table: set_state says so and the engine refuses to step
    bent = B["pos"].copy()
    bent[3 * 11 + 1] += 0.03 * (B["unwrapped"][3 * 11 + 1] - B["unwrapped"][3 * 11])   # (leg a of molecule 11, 3 % farther out)
    text = _refused(E, ERR_STATE, md.set_state_, E.cu(bent, dev), E.cu(raw, dev), E.cu(ghostly, dev), E.cu(1.0 / B["mass"], dev))
    assert "molecule 11 " in text
    _refused(E, ERR_STATE, md.step_, 1, DT)
    # another count
    load(447, raw)
    _refused(E, ERR_STATE, md.step_, 1, DT)
    md.set_rigid3_(B["mol"][:149], B["geom"][:149])
    md.step_(2, DT)
    load(450, raw)
    _refused(E, ERR_STATE, md.step_, 1, DT)
    md.set_rigid3_(None, None)                                               # cleared: steps again
    md.step_(1, DT)
    md.close()


def test_a_move_too_far_is_an_error_return_naming_the_molecule(emdee, dev):
    E = emdee
    B = sr.water_box()
    vel = B["vel"].copy()
    vel[3 * 17:3 * 17 + 3] = 1e3 * np.eye(3)                                 # three different directions: no rigid motion
    md = _engine(E, dev, B, vel=vel)
    text = _refused(E, ERR_STATE, md.step_, 1, DT)
    assert "molecule 17 " in text and "atoms 51 52 53" in text
    _refused(E, ERR_STATE, md.step_, 1, DT)                                  # refused until the table or the state is replaced
    md.set_state_(E.cu(B["pos"], dev), E.cu(B["vel"], dev), E.cu(B["atoms"], dev), E.cu(1.0 / B["mass"], dev))
    md.step_(3, DT)
    _constraints_hold(md, B, np.float64, "after the error and a new state")
    md.close()
