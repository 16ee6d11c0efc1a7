"""GPU tests of bonds to hydrogen at fixed lengths (include/emdee_hip.h: emdee_md_set_hbonds; csrc/shake.hpp) against the numpy
yardstick of tests/helpers/shake_ref.py: Gauss-Seidel SHAKE and RATTLE around a force callback, no Newton / matrix form.

One small box for all of them (shake_ref.mixed_box): 300 star clusters (100 each of 2, 3 and 4 atoms; masses (12, 1.008), (14,
1.008) and the inverted (1, 19); distances between 0.28 and 0.40), 60 rigid waters of settle_ref's geometry and 100 free atoms,
1180 atoms in a box of sides (9.0, 9.6, 10.5) at lo = (-1.0, 0.5, 2.0), rc = 2.5, skin = 0.4 (three cells per side), the pairs
within a cluster and within a water excluded, every atom wrapped on its own so that groups straddle box faces and cell faces,
velocities projected by the reference, dt = 0.002."""
import numpy as np
import pytest

from .helpers import shake_ref as hr
from .test_gpu_dd_pairs import _build

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
DT = hr.DT
EPS32 = float(np.finfo(np.float32).eps)


@pytest.fixture
def dev():
    return torch.device("cuda", 0)


def _engine(E, dev, B, dtype=np.float64, masses=True, excl=True, hbonds=True, rigid=False, vel=None, atoms=None):
    im = E.cu((1.0 / B["mass"]).astype(dtype), dev) if masses else None
    vel = B["vel"] if vel is None else vel
    md = E.VelocityVerlet(E.cu(B["pos"].astype(dtype), dev), E.cu(np.asarray(vel).astype(dtype), dev), float(hr.LENGTHS[0]),
                          E.LennardJonesModel(hr.RC, hr.RS), E.cu(B["atoms"] if atoms is None else atoms, dev), skin=hr.SKIN, inv_mass=im,
                          lo=list(hr.LO), lengths=list(hr.LENGTHS), periodic=[1, 1, 1])
    if excl:
        md.set_exclusions_(B["excl"])
    if hbonds:
        md.set_hbonds_(B["clusters"], B["dist"])
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


def _against_reference(md, x_start, v_start, offset, B, pairs, checkpoints, rebuild_every, what):
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
    hr.constrained_verlet(x_start, v_start, force, max(checkpoints), DT, pairs, B["mass"], observe=observe)
    for s in checkpoints:
        ex, ev, vrms = seen[s]
        print("%s, step %d: max |dx| = %.3e (box side %.1f), max |dv| = %.3e (rms velocity %.3f)" % (what, s, ex, hr.LENGTHS.max(), ev, vrms))
        assert ex <= 1e-11 * hr.LENGTHS.max() and ev <= 1e-11 * vrms, (what, s, ex, ev)


def _constraints_hold(md, B, pairs, dtype, what, records=False, relative=False):
    """every distance and every bond-relative velocity of the engine's state within the bounds of test_gpu_settle: 1e-12 in fp64;
    in fp32 8 ulp_fp32(L_max) / d for a distance d (the rounding of the caller-order positions get_state returns) and 8 eps_fp32
    for the velocities, to which cell-relative records (relative: read through caller-order positions, each off by up to
    ulp_fp32(L_max) / 2 per axis) add 2 sqrt(3) ulp_fp32(L_max) / d"""
    x, v = _xv(md)
    u = hr.unwrap(x, pairs, hr.LENGTHS)
    i, j, d = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64), pairs[:, 2]
    res = np.abs(np.linalg.norm(u[i] - u[j], axis=1) / d - 1.0)
    if dtype == np.float64:
        tol_x, tol_v = np.full(len(d), 1e-12), np.full(len(d), 1e-12)
    else:
        ulp = float(np.spacing(np.float32(np.abs(x).max())))
        tol_x = 8.0 * ulp / d
        tol_v = 8.0 * EPS32 + (2.0 * np.sqrt(3.0) * ulp / d if relative else 0.0 * d)
    if records:
        # Float32 with masses keeps absolute records: pack_positions with a zero shift returns them as they are, the geometry
        # stage (e) itself used, without the rounding of record + box lengths in get_state
        ids = torch.arange(x.shape[0], dtype=torch.int32, device=md.device)
        u = hr.unwrap(md.pack_positions(ids, [0.0, 0.0, 0.0]).cpu().numpy().astype(np.float64), pairs, hr.LENGTHS)
    left = hr.bond_velocities(u, v, pairs)
    print("%s: largest relative distance error %.3e (%.2f of its bound), largest bond-relative velocity / (|v| d) %.3e (%.2f of its bound)"
          % (what, res.max(), (res / tol_x).max(), left.max(), (left / tol_v).max()))
    assert (res <= tol_x).all() and (left <= tol_v).all(), (what, res.max(), left.max())


# ---------------------------------------------------------------- 1. against the reference
@pytest.mark.parametrize("waters", [False, True], ids=["clusters", "clusters+waters"])
def test_one_step_and_twenty_steps_match_the_reference(emdee, dev, waters):
    # (with the clusters alone the waters are free atoms whose mutual pairs are excluded: 20 such steps are harmless)
    B = hr.mixed_box()
    md = _engine(emdee, dev, B, rigid=waters)
    pairs = B["pairs"] if waters else B["pairs_h"]
    _against_reference(md, B["unwrapped"], B["vel"], B["pos"] - B["unwrapped"], B, pairs, (1, 20), 3, "fp64, rebuild_every = 3")
    assert md.nbr_stats()["builds"] >= 1 + 20 // 3                           # (re-sorts fell between the two stages)
    md.close()


# ---------------------------------------------------------------- 2. the constraints hold
@pytest.mark.parametrize("langevin", [False, True], ids=["nve", "langevin"])
@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["f64", "f32"])
def test_constraints_hold_over_300_steps_with_automatic_rebuilds(emdee, dev, dtype, langevin):
    B = hr.mixed_box()
    md = _engine(emdee, dev, B, dtype, rigid=True)
    if langevin:
        md.set_langevin_(1.0, 1.0, seed=7)
    before = md.nbr_stats()["builds"]
    md.step_(300, DT)
    assert md.nbr_stats()["builds"] > before
    _constraints_hold(md, B, B["pairs"], dtype, "%s, %s" % (np.dtype(dtype).name, "Langevin" if langevin else "NVE"), records=dtype == np.float32)
    md.close()


def test_constraints_hold_on_cell_relative_float32_records(emdee, dev):
    # Float32 without masses keeps cell-relative records (kernels.hpp RelGrid): the stages add the cells' origins in double.  All
    # masses 1.
    B = hr.mixed_box()
    B["mass"] = np.ones_like(B["mass"])
    B["vel"] = hr.rattle(B["unwrapped"], B["vel"], B["pairs"], B["mass"])
    md = _engine(emdee, dev, B, np.float32, masses=False, rigid=True)
    before = md.nbr_stats()["builds"]
    md.step_(300, DT)
    assert md.nbr_stats()["builds"] > before
    _constraints_hold(md, B, B["pairs"], np.float32, "f32 cell-relative", relative=True)
    md.close()


# ---------------------------------------------------------------- 3. dealing, reproducibility, the timer
def test_dealing_of_steps_to_calls_and_reruns_are_bit_identical(emdee, dev):
    B = hr.mixed_box()
    out = []
    for deal in ((40,), (5,) * 8, (1,) * 40, (40,)):
        md = _engine(emdee, dev, B, rigid=True)
        md.profile_(True)
        for n in deal:
            md.step_(n, DT)
        out.append(_xv(md))
        ms, launches = md.kernel_time("hbonds")
        assert launches == 3 * 40 and ms > 0.0                               # (stages (a), (c), (e) of every step; emdee_md_kernel_time index 11)
        assert md.kernel_time("settle")[1] == 3 * 40
        md.close()
    for x, v in out[1:]:
        assert np.array_equal(x, out[0][0]) and np.array_equal(v, out[0][1])


def test_kernel_time_index_11_is_zero_without_a_table(emdee, dev):
    E = emdee
    B = hr.mixed_box()
    md = _engine(E, dev, B, hbonds=False, rigid=True)
    md.profile_(True)
    md.step_(3, DT)
    assert md.kernel_time("hbonds") == (0.0, 0) and md.kernel_time("settle")[1] == 9
    # (the clusters have drifted off their distances meanwhile: the table goes on the starting state again)
    md.set_state_(E.cu(B["pos"], dev), E.cu(B["vel"], dev), E.cu(B["atoms"], dev), E.cu(1.0 / B["mass"], dev))
    md.set_hbonds_(B["clusters"], B["dist"])
    assert md.kernel_time("hbonds")[1] == 1                                  # (the call's one velocity stage)
    md.step_(3, DT)
    ms, launches = md.kernel_time("hbonds")
    assert launches == 10 and ms > 0.0
    md.close()


def test_every_stage_runs_once_per_table_and_step_under_its_own_timer(emdee, dev):
    # Both tables in force: stages (a), (c), (e) of every step run once for the molecules (index 9) and once for the clusters
    # (index 11), and nothing is booked on the molecular sums (index 10).
    md = _engine(emdee, dev, hr.mixed_box(), rigid=True)
    md.profile_(True)
    md.step_(5, DT)
    assert md.kernel_time("settle")[1] == 3 * 5
    assert md.kernel_time("hbonds")[1] == 3 * 5
    assert md.kernel_time("molecular") == (0.0, 0)
    md.close()


def test_clearing_the_table_restores_the_unconstrained_trajectory(emdee, dev):
    # The pairs within a cluster are excluded and nothing else holds it together: 20 unconstrained steps are harmless.
    # Installing the table projects the velocities, so the twin that never had one starts from the state the install left.
    B = hr.mixed_box()
    md = _engine(emdee, dev, B)
    x, v = _xv(md)
    assert np.array_equal(x, B["pos"])                                       # (the call moved no atom)
    md.set_hbonds_(None, None)
    twin = _engine(emdee, dev, B, hbonds=False, vel=v)
    md.step_(20, DT)
    twin.step_(20, DT)
    (xa, va), (xb, vb) = _xv(md), _xv(twin)
    assert np.array_equal(xa, xb) and np.array_equal(va, vb)
    assert hr.residual(hr.unwrap(xa, B["pairs_h"], hr.LENGTHS), B["pairs_h"]) > 1e-6      # (and it is unconstrained)
    md.close()
    twin.close()


# ---------------------------------------------------------------- 4. charged engines
def test_charged_engine_with_reaction_field_then_pme(emdee, dev):
    B = hr.mixed_box()
    md = _engine(emdee, dev, B, hbonds=False)
    md.set_coulomb_(B["charges"], 1.0)
    md.set_hbonds_(B["clusters"], B["dist"])
    md.set_rigid3_(B["mol"], B["geom"])
    _against_reference(md, B["unwrapped"], B["vel"], B["pos"] - B["unwrapped"], B, B["pairs"], (1,), 0, "reaction field")
    md.step_(49, DT)
    _constraints_hold(md, B, B["pairs"], np.float64, "reaction field, 50 steps")
    md.set_pme_(1.2, 16, 4)
    x, v = _xv(md)
    u = hr.unwrap(x, B["pairs"], hr.LENGTHS)
    _against_reference(md, u, v, x - u, B, B["pairs"], (1,), 0, "PME")
    md.step_(49, DT)
    _constraints_hold(md, B, B["pairs"], np.float64, "PME, 50 steps")
    md.close()


# ---------------------------------------------------------------- 5. refusals and state rules
def test_invalid_tables_are_refused_and_the_previous_table_still_steps(emdee, dev):
    E = emdee
    B = hr.mixed_box()
    md = _engine(E, dev, B, rigid=True)
    cl, dist, n_atoms = B["clusters"], B["dist"], B["pos"].shape[0]
    assert cl[0, 2] == -1 and cl[1, 3] == -1 and cl[2, 3] >= 0               # (clusters of 2, 3 and 4 atoms in turn)

    def changed(arr, m, k, value):
        out = arr.astype(np.float64 if arr is dist else np.int64).copy()
        out[m, k] = value
        return out
    one = torch.zeros(4, dtype=torch.int32, device=dev)
    cases = {
        "NULL atoms": lambda: E._lib.call("emdee_md_set_hbonds", md._handle, None, None, 1),
        "NULL dist": lambda: E._lib.call("emdee_md_set_hbonds", md._handle, one.data_ptr(), None, 1),
        "negative count": lambda: E._lib.call("emdee_md_set_hbonds", md._handle, one.data_ptr(), one.data_ptr(), -1),
        "id too high": lambda: md.set_hbonds_(changed(cl, 3, 1, n_atoms), dist),
        "negative centre": lambda: md.set_hbonds_(changed(cl, 3, 0, -1), dist),
        "id below -1": lambda: md.set_hbonds_(changed(cl, 4, 3, -2), dist),
        "empty cluster": lambda: md.set_hbonds_(changed(cl, 3, 1, -1), dist),
        "an id after a -1": lambda: md.set_hbonds_(changed(cl, 5, 2, -1), dist),       # (cluster 5 has four atoms)
        "twice within": lambda: md.set_hbonds_(changed(cl, 5, 2, cl[5, 0]), dist),
        "twice across": lambda: md.set_hbonds_(changed(cl, 5, 2, cl[9, 1]), dist),
        "named by the rigid table": lambda: md.set_hbonds_(changed(cl, 5, 2, B["mol"][7, 1]), dist),
        "nan distance": lambda: md.set_hbonds_(cl, changed(dist, 2, 0, np.nan)),
        "infinite distance": lambda: md.set_hbonds_(cl, changed(dist, 2, 1, np.inf)),
        "zero distance": lambda: md.set_hbonds_(cl, changed(dist, 2, 2, 0.0)),
        "negative distance": lambda: md.set_hbonds_(cl, changed(dist, 1, 1, -0.3)),
        # the mirror case: a molecule of the rigid table that names an atom of a cluster
        "rigid table names a cluster's atom": lambda: md.set_rigid3_(changed(B["mol"], 7, 1, cl[5, 2]), B["geom"]),
    }
    for name, call in cases.items():
        text = _refused(E, ERR_INVALID, call)
        if "rigid" in name:
            assert "in force" in text, text
        md.step_(1, DT)
    with pytest.raises(ValueError):
        md.set_hbonds_(cl[:, :3], dist)                                      # (the binding's shape check)
    with pytest.raises(ValueError):
        md.set_hbonds_(cl, dist[:-1])
    md.set_hbonds_(cl, changed(dist, 0, 2, np.nan))                          # (the distance of an unused slot is ignored)
    # the device check: a distance 3 % off
    text = _refused(E, ERR_STATE, md.set_hbonds_, cl, changed(dist, 5, 1, 1.03 * dist[5, 1]))
    assert "cluster 5 " in text and "distance" in text and "atoms %d %d %d %d" % tuple(cl[5]) in text
    md.step_(1, DT)
    # pressure: refused whatever the molecular switch says
    for molecular in (False, True):
        md.set_molecular_scaling_(molecular)
        assert "emdee_md_set_hbonds" in _refused(E, ERR_STATE, md.scale_box_, 1.001)
        assert "emdee_md_set_hbonds" in _refused(E, ERR_STATE, md.set_barostat_, E.BAROSTAT_BERENDSEN, 1.0, 0.01, 1.0, 5)
        assert "emdee_md_set_hbonds" in _refused(E, ERR_STATE, md.molecular_tensor_sums)
        md.set_barostat_(E.BAROSTAT_OFF)
        md.step_(1, DT)
    md.set_molecular_scaling_(False)
    _constraints_hold(md, B, B["pairs"], np.float64, "after %d refusals" % (len(cases) + 9))     # (the tables set at the start are in force)
    md.close()
    # set_hbonds under a barostat, with the molecular switch off and on
    other = _engine(E, dev, B, hbonds=False)
    for molecular in (False, True):
        other.set_molecular_scaling_(molecular)
        other.set_barostat_(E.BAROSTAT_BERENDSEN, 1.0, 0.01, 1.0, 5)
        assert "emdee_md_set_barostat" in _refused(E, ERR_STATE, other.set_hbonds_, cl, dist)
        other.set_barostat_(E.BAROSTAT_OFF)
    other.set_hbonds_(cl, dist)
    other.step_(2, DT)
    # the other call order of the overlap: the clusters are in force, the rigid table comes second
    _refused(E, ERR_INVALID, other.set_rigid3_, changed(B["mol"], 7, 1, cl[5, 2]), B["geom"])
    other.set_rigid3_(B["mol"], B["geom"])
    other.step_(2, DT)
    _constraints_hold(other, B, B["pairs"], np.float64, "the second engine")
    other.close()


def test_an_engine_lent_by_a_decomposition_refuses_the_call(emdee, dev):
    E = emdee
    pos, gid, lengths = E.synthetic.fcc_block((8,) * 3, (0, 0, 0), (8,) * 3)             # (two bricks of rc + skin + halo)
    pos = pos[np.argsort(gid)]
    N = pos.shape[0]
    dd = _build(E, 2, pos, np.zeros((N, 3)), E.lennard_jones_atoms(1.0, 1.0, N), float(lengths[0]))
    text = _refused(E, ERR_STATE, dd.engine(0).set_hbonds_, [[0, 1, -1, -1]], [[1.0, 0.0, 0.0]])
    assert "emdee_dd_engine" in text
    dd.step_(2, 0.005)                                                                   # the decomposition is unharmed
    dd.close()


def test_set_state_keeps_the_table_for_the_same_count_and_refuses_to_step_for_another(emdee, dev):
    # without exclusions (they would refuse the smaller state themselves) and without LJ forces (twice_sqrt_eps = 0): the rules
    # of the table alone.  The clusters are the first 900 atoms.
    E = emdee
    B = hr.mixed_box()
    ghostly = B["atoms"].copy()
    ghostly["twice_sqrt_eps"] = 0.0
    n_all, cl, pairs = B["pos"].shape[0], B["clusters"], B["pairs_h"]
    md = _engine(E, dev, B, excl=False, atoms=ghostly)
    rng = np.random.default_rng(3)
    raw = rng.normal(size=B["vel"].shape)                                    # velocities with bond components
    load = lambda n, vel: md.set_state_(E.cu(B["pos"][:n], dev), E.cu(vel[:n], dev), E.cu(ghostly[:n], dev), E.cu(1.0 / B["mass"][:n], dev))
    load(n_all, raw)
    x, v = _xv(md)
    assert hr.bond_velocities(hr.unwrap(x, pairs, hr.LENGTHS), v, pairs).max() <= 1e-12            # (checked and projected again)
    assert np.abs(v - hr.rattle(B["unwrapped"], raw, pairs, B["mass"])).max() <= 1e-12 * np.abs(raw).max()
    md.step_(5, DT)
    _constraints_hold(md, B, pairs, np.float64, "after set_state with the same count")
    # the same count, a state that does not fit the table: set_state says so and the engine refuses to step
    bent = B["pos"].copy()
    c, s = cl[11, 0], cl[11, 1]
    bent[s] += 0.03 * (B["unwrapped"][s] - B["unwrapped"][c])                # (the first satellite of cluster 11, 3 % farther out)
    text = _refused(E, ERR_STATE, md.set_state_, E.cu(bent, dev), E.cu(raw, dev), E.cu(ghostly, dev), E.cu(1.0 / B["mass"], dev))
    assert "cluster 11 " in text
    _refused(E, ERR_STATE, md.step_, 1, DT)
    # another count
    load(n_all - 3, raw)
    _refused(E, ERR_STATE, md.step_, 1, DT)
    md.set_hbonds_(cl[:299], B["dist"][:299])
    md.step_(2, DT)
    load(n_all, raw)
    _refused(E, ERR_STATE, md.step_, 1, DT)
    md.set_hbonds_(None, None)                                               # cleared: steps again
    md.step_(1, DT)
    md.close()


def test_a_move_without_a_solution_is_an_error_return_naming_the_cluster(emdee, dev):
    # The satellite of cluster 9 (two atoms, masses 12 and 1.008) gets a velocity that carries it 1.5 d across its bond in one
    # step: corrections along the bond of x0 cannot bring it back within d.  An error return, not a fault.
    E = emdee
    B = hr.mixed_box()
    c, s = B["clusters"][9, 0], B["clusters"][9, 1]
    assert B["clusters"][9, 2] == -1 and B["mass"][c] == 12.0
    bond = B["unwrapped"][s] - B["unwrapped"][c]
    across = np.cross(bond, [0.3, -0.5, 0.8])
    vel = B["vel"].copy()
    vel[s] = vel[c] + 1.5 * B["dist"][9, 0] / DT * across / np.linalg.norm(across)
    md = _engine(E, dev, B, vel=vel, hbonds=False)
    md.set_hbonds_(B["clusters"], B["dist"])                                 # (the velocity is across the bond: the projection keeps it)
    text = _refused(E, ERR_STATE, md.step_, 1, DT)
    assert "cluster 9 " in text and "atoms %d %d)" % (c, s) in text
    x, _ = _xv(md)
    u = hr.unwrap(x, B["pairs_h"], hr.LENGTHS)
    far = np.linalg.norm(u[s] - u[c]) / B["dist"][9, 0]
    assert 1.7 <= far <= 1.9                                                 # (left where the drift put it: sqrt(1 + 1.5^2) d)
    others = np.delete(B["pairs_h"], np.where(B["pairs_h"][:, 0] == c)[0], axis=0)
    assert hr.residual(u, others) <= 1e-12                                   # (every other cluster was solved)
    _refused(E, ERR_STATE, md.step_, 1, DT)                                  # refused until the table or the state is replaced
    md.set_state_(E.cu(B["pos"], dev), E.cu(B["vel"], dev), E.cu(B["atoms"], dev), E.cu(1.0 / B["mass"], dev))
    md.step_(3, DT)
    _constraints_hold(md, B, B["pairs_h"], np.float64, "after the error and a new state")
    md.close()
