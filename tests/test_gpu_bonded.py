"""GPU tests of the bonded terms (emdee_md_set_bonded / emdee_dd_set_bonded): harmonic bonds, harmonic angles and periodic
torsions evaluated owner-computes behind every force pass, their partners found through the neighbour rows.  The yardsticks
are the oracle's LJ sum minus the named pairs plus the scaled 1-4 terms (as tests/test_gpu_dd_pairs.py) plus the numpy
restatement of the bonded terms in tests/helpers/bonded_ref.py, and the undivided integrator for decomposed runs."""
import numpy as np
import pytest

from .helpers import bonded_ref as br
from .test_gpu_dd_pairs import _build, _compare, _gather, _global_box, _lj14scale, _pair_terms

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RC, RS, SKIN, DT = 2.5, 2.0, 0.3, 0.005
ERR_INVALID, ERR_STATE = -1, -6
BOND_P, ANGLE_P = (200.0, 0.95), (40.0, 1.2)
TORSION_P = ((1.5, 1.0, 0.0), (0.6, 3.0, np.pi))


def _chains(N):
    """Chain 'molecules' of the four atoms of each fcc cell: bonds 0-1, 1-2, 2-3, angles 0-1-2, 1-2-3, the torsion 0-1-2-3
    with two terms; 1-2 and 1-3 pairs excluded, the 1-4 pair scaled."""
    mol = np.arange(N).reshape(-1, 4)
    bonds = np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]], mol[:, [2, 3]]])
    angles = np.concatenate([mol[:, [0, 1, 2]], mol[:, [1, 2, 3]]])
    tors = np.concatenate([mol, mol])
    tp = np.concatenate([np.tile(TORSION_P[0], (len(mol), 1)), np.tile(TORSION_P[1], (len(mol), 1))])
    terms = [(br.BOND, bonds, np.tile(BOND_P, (len(bonds), 1))), (br.ANGLE, angles, np.tile(ANGLE_P, (len(angles), 1))),
             (br.TORSION, tors, tp)]
    excl = np.concatenate([mol[:, [0, 1]], mol[:, [1, 2]], mol[:, [2, 3]], mol[:, [0, 2]], mol[:, [1, 3]]])
    return terms, excl, mol[:, [0, 3]]


def _box(E, ncell=8, uniform=False):
    """tests/test_gpu_dd_pairs.py's box shifted by 0.75 of a cell and wrapped: the molecules of the last cells cross the edge
    (and those next to a domain cut cross the cut)."""
    pos, vel, eps, sigma, L = _global_box(E.synthetic, uniform=uniform, ncell=ncell)
    pos = np.mod(pos + 0.75 * L / ncell, L)
    return pos, vel, eps, sigma, L


def _md(E, pos, vel, atoms, L, dtype=torch.float64, excl=None, p14=None, s14=1.0, terms=None, inv_mass=None, rc=RC, rs=RS,
        skin=SKIN):
    dev = torch.device("cuda", 0)
    ndt = np.float64 if dtype == torch.float64 else np.float32
    im = None if inv_mass is None else E.cu(inv_mass.astype(ndt), dev)
    md = E.VelocityVerlet(E.cu(pos.astype(ndt), dev), E.cu(vel.astype(ndt), dev), L, E.LennardJonesModel(rc, rs), E.cu(atoms, dev),
                          skin=skin, inv_mass=im)
    if excl is not None:
        md.set_exclusions_(excl)
    if p14 is not None:
        md.set_pairs14_(p14, s14)
    for kind, a, p in terms or []:
        md.set_bonded_(kind, a, p)
    return md


def _outputs(md):
    st = md.state(positions=False, velocities=False, energies=True, virials=True)
    out = [st["forces"], st["energies"], st["virials"], md.virial_tensor()]
    return [t.cpu().numpy().astype(np.float64) for t in out] + [np.array(md.tensor_sums()[:6])]


def _reference(oracle, pos, L, atoms, excl, p14, s14, terms, rc=RC, rs=RS):
    om = oracle.model(rc, rs)
    f0, e0, w0 = oracle.nonbonded_cells(np.mod(pos, L), L, om, atoms)
    fx, ex, wx = _pair_terms(oracle, pos, L, om, atoms, excl)
    f4, e4, w4 = _pair_terms(oracle, pos, L, om, atoms, p14)
    fb, eb, wb, tb = br.bonded(pos, L, terms)
    return (f0 - fx - (1 - s14) * f4 + fb, e0 - ex - (1 - s14) * e4 + eb, w0 - wx - (1 - s14) * w4 + wb), (fb, eb, wb, tb)


def _check_bonded_part(with_b, without, ref, tol):
    fb, eb, wb, tb = ref
    for got, want in zip([a - b for a, b in zip(with_b[:4], without[:4])], [fb, eb, wb, tb]):
        assert np.abs(got - want).max() <= tol * np.abs(want).max()
    # the box sums of the tensor (emdee_md_pressure_tensor's first six)
    tsum = tb.sum(axis=0)
    assert np.abs((with_b[4] - without[4]) - tsum).max() <= tol * np.abs(tsum).max() * 10


@pytest.mark.parametrize("path,dtype", [("brick", torch.float64), ("direct", torch.float64), ("brick", torch.float32)])
def test_chains_at_the_load_match_the_oracle_and_the_reference(emdee, oracle, monkeypatch, path, dtype):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    pos, vel, eps, sigma, L = _box(E)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    s14 = _lj14scale(E)
    if dtype == torch.float32:
        pos = pos.astype(np.float32).astype(np.float64)
    span = np.abs(pos.reshape(-1, 4, 1, 3) - pos.reshape(-1, 1, 4, 3)).max(axis=(1, 2, 3))
    assert (span > L / 2).any()                                        # some molecules cross the box edge
    md = _md(E, pos, vel, atoms, L, dtype=dtype, excl=excl, p14=p14, s14=s14)
    without = _outputs(md)
    for kind, a, p in terms:
        md.set_bonded_(kind, a, p)
    with_b = _outputs(md)
    (want_f, want_e, want_w), ref = _reference(oracle, pos, L, atoms, excl, p14, s14, terms)
    _check_bonded_part(with_b, without, ref, 1e-9 if dtype == torch.float64 else 1e-4)
    tol = 1e-6 if dtype == torch.float64 else 1e-4
    assert np.abs(with_b[0] - want_f).max() <= tol * np.abs(want_f).max()
    assert np.abs(with_b[1] - want_e).max() <= tol * np.abs(want_e).max()
    assert np.abs(with_b[2] - want_w).max() <= tol * np.abs(want_w).max()
    ep, _, vir = md.totals()
    assert ep == pytest.approx(want_e.sum(), rel=tol) and vir == pytest.approx(want_w.sum(), rel=tol)
    # per-atom tensors: trace = virial
    assert np.abs(with_b[3][:, :3].sum(axis=1) - with_b[2]).max() <= tol * np.abs(want_w).max()
    md.close()


def test_water_box_matches_the_oracle_and_the_reference(emdee, oracle):
    E = emdee
    w = E.synthetic.water_box(10)
    L, atoms, inv_mass = w["L"], w["atoms"], w["inv_mass"]
    N = w["positions"].shape[0]
    # off the tables' r0 and theta0, so that every term has a force
    pos = np.mod(w["positions"] + np.random.default_rng(7).uniform(-0.005, 0.005, (N, 3)), L)
    vel = np.zeros((N, 3))
    rc, rs = 1.0, 0.9
    terms = [(br.BOND, w["bonds"], w["bond_params"]), (br.ANGLE, w["angles"], w["angle_params"])]
    excl = w["exclusions"]
    md = _md(E, pos, vel, atoms, L, excl=excl, inv_mass=inv_mass, rc=rc, rs=rs, skin=0.1)
    without = _outputs(md)
    for kind, a, p in terms:
        md.set_bonded_(kind, a, p)
    with_b = _outputs(md)
    (want_f, want_e, want_w), ref = _reference(oracle, pos, L, atoms, excl, np.zeros((0, 2), dtype=int), 1.0, terms, rc=rc, rs=rs)
    _check_bonded_part(with_b, without, ref, 1e-9)
    assert np.abs(with_b[0] - want_f).max() <= 1e-6 * np.abs(want_f).max()
    assert np.abs(with_b[1] - want_e).max() <= 1e-6 * np.abs(want_e).max()
    md.close()


def _numpy_verlet(oracle, pos, vel, L, atoms, excl, p14, s14, terms, nsteps, dt):
    x, v = pos.copy(), vel.copy()
    f = _reference(oracle, x, L, atoms, excl, p14, s14, terms)[0][0]
    for _ in range(nsteps):
        v += 0.5 * dt * f
        x += dt * v
        f = _reference(oracle, x, L, atoms, excl, p14, s14, terms)[0][0]
        v += 0.5 * dt * f
    return x, v


def test_trajectory_matches_a_numpy_velocity_verlet(emdee, oracle):
    E = emdee
    pos, vel, eps, sigma, L = _box(E, ncell=6)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    s14 = _lj14scale(E)
    md = _md(E, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14, terms=terms)
    md.step_(50, DT)
    x = md.state()["positions"].cpu().numpy()
    xr, _ = _numpy_verlet(oracle, pos, vel, L, atoms, excl, p14, s14, terms, 50, DT)
    d = x - xr
    assert np.abs(d - L * np.rint(d / L)).max() < 1e-8
    md.close()


def test_energy_fluctuation_scales_as_dt_squared(emdee):
    E = emdee
    pos, vel, eps, sigma, L = _box(E, ncell=6)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    s14 = _lj14scale(E)
    rms = []
    for dt, every in ((0.004, 1), (0.002, 2)):
        md = _md(E, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14, terms=terms)
        tot = []
        for _ in range(100):
            md.step_(every, dt)
            ep, ek, _ = md.totals()
            tot.append(ep + ek)
        rms.append(np.std(tot))
        md.close()
    assert 3.0 <= rms[0] / rms[1] <= 5.0, rms


def test_invalid_bonded_tables_are_refused(emdee):
    E = emdee
    pos, vel, eps, sigma, L = _box(E, ncell=6)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    md = _md(E, pos, vel, atoms, L, excl=excl, terms=terms)
    f0 = md.state()["forces"].cpu().numpy()
    bad = [(99, [[0, 1]], [[1.0, 1.0]]),                                   # unknown kind
           (E.HARMONIC_BOND, [[0, 0]], [[1.0, 1.0]]),                      # an atom twice
           (E.HARMONIC_ANGLE, [[0, 1, 0]], [[1.0, 1.0]]),
           (E.HARMONIC_BOND, [[0, N]], [[1.0, 1.0]]),                      # out of range
           (E.HARMONIC_BOND, [[-1, 1]], [[1.0, 1.0]]),
           (E.HARMONIC_BOND, [[0, 1]], [[np.nan, 1.0]]),                   # non-finite
           (E.HARMONIC_BOND, [[0, 1]], [[1.0, -0.1]]),                     # r0 < 0
           (E.HARMONIC_ANGLE, [[0, 1, 2]], [[1.0, 3.2]]),                  # theta0 > pi
           (E.HARMONIC_ANGLE, [[0, 1, 2]], [[1.0, -0.1]]),
           (E.PERIODIC_TORSION, [[0, 1, 2, 3]], [[1.0, 1.5, 0.0]]),        # n not an integer
           (E.PERIODIC_TORSION, [[0, 1, 2, 3]], [[1.0, 0.0, 0.0]]),        # n < 1
           (E.PERIODIC_TORSION, [[0, 1, 2, 3]], [[1.0, 2.0, np.inf]])]
    for kind, a, p in bad:
        with pytest.raises(E.EmDeeError) as err:
            md.set_bonded_(kind, a, p)
        assert err.value.code == ERR_INVALID, (kind, a, p)
    # a NULL array with n > 0, through the C ABI
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_set_bonded", md._handle, 1, None, None, 3)
    assert err.value.code == ERR_INVALID
    md.forces_()
    assert np.array_equal(md.state()["forces"].cpu().numpy(), f0)
    # a bond longer than rc + skin: refused from the set call, and the engine refuses to step
    far = np.argmax(np.linalg.norm(np.mod(pos - pos[0] + L / 2, L) - L / 2, axis=1))
    with pytest.raises(E.EmDeeError) as err:
        md.set_bonded_(E.HARMONIC_BOND, [[0, far]], [[1.0, 1.0]])
    assert err.value.code == ERR_STATE and "bond 0" in str(err.value)
    with pytest.raises(E.EmDeeError) as err:
        md.step_(1, DT)
    assert err.value.code == ERR_STATE
    md.set_bonded_(E.HARMONIC_BOND, terms[0][1], terms[0][2])         # replaced: steps again
    md.step_(2, DT)
    md.close()


def test_a_partner_that_drifts_away_is_reported_by_the_next_step_call(emdee):
    E = emdee
    pos, vel, eps, sigma, L = _box(E, ncell=6)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    # a weak bond between two atoms 2.6 apart (inside rc + skin), the second one flying off
    d = np.linalg.norm(np.mod(pos - pos[0] + L / 2, L) - L / 2, axis=1)
    j = int(np.argmin(np.abs(d - 2.6)))
    vel = vel.copy()
    vel[j] = 40.0 * (np.mod(pos[j] - pos[0] + L / 2, L) - L / 2) / d[j]
    md = _md(E, pos, vel, atoms, L, terms=[(br.BOND, [[0, j]], [[0.0, 2.6]])])
    with pytest.raises(E.EmDeeError) as err:
        md.step_(40, DT, 5)
    assert err.value.code == ERR_STATE and "bond 0" in str(err.value)
    with pytest.raises(E.EmDeeError) as err:
        md.step_(1, DT)
    assert err.value.code == ERR_STATE
    md.close()


def test_lent_engines_refuse_set_bonded(emdee):
    E = emdee
    pos, vel, eps, sigma, L = _box(E)
    atoms = E.lennard_jones_atoms(eps, sigma)
    dd = _build(E, 2, pos, vel, atoms, L)
    with pytest.raises(E.EmDeeError) as err:
        dd.engine(0).set_bonded_(E.HARMONIC_BOND, [[0, 1]], [[1.0, 1.0]])
    assert err.value.code == ERR_STATE
    dd.close()


def test_no_bonded_tables_keep_the_fused_step(emdee):
    E = emdee
    pos, vel, eps, sigma, L = _box(E)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, _ = _chains(N)
    md = _md(E, pos, vel, atoms, L, excl=excl)
    md.profile_(True)
    md.step_(60, DT)
    assert md.kernel_time("lj_force_nbr_fused_step")[1] >= 50
    md.set_bonded_(E.HARMONIC_BOND, terms[0][1], terms[0][2])
    md.profile_(True)
    md.step_(60, DT)
    assert md.kernel_time("lj_force_nbr_fused_step")[1] == 0
    assert md.kernel_time("verlet_kick_drift")[1] >= 59
    md.close()


@pytest.mark.parametrize("world,rebuild_every,variant", [(2, 0, "f64"), (4, 0, "f64"), (8, 0, "f64"), (2, 6, "f64"), (8, 5, "f64"),
                                                         (8, 0, "f32"), (4, 0, "langevin")])
def test_decomposed_chains_match_the_undivided_run(emdee, world, rebuild_every, variant):
    E = emdee
    dtype = torch.float32 if variant == "f32" else torch.float64
    pos, vel, eps, sigma, L = _box(E)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    s14 = _lj14scale(E)
    dd = _build(E, world, pos, vel, atoms, L, dtype=dtype, excl=excl, p14=p14, s14=s14, load=False)
    for kind, a, p in terms:
        dd.set_bonded_(kind, a, p)
    dd.load_()
    md = _md(E, pos, vel, atoms, L, dtype=dtype, excl=excl, p14=p14, s14=s14, terms=terms)
    if variant == "langevin":
        dd.set_langevin_(2.0, 0.7, 0x5EED)
        md.set_langevin_(2.0, 0.7, 0x5EED)
    _, _, _, owner = _gather(dd, world, N)
    tors = terms[2][1]
    assert (owner[tors] != owner[tors[:, :1]]).any()                 # some terms span domains
    dd.step_(29, DT, rebuild_every)
    dd.step_(31, DT, rebuild_every)
    md.step_(60, DT, rebuild_every)
    if dtype == torch.float32:
        _compare(dd, md, world, N, L, tol_x=2e-4, tol_v=2e-3, tol_e=1e-4)
    else:
        _compare(dd, md, world, N, L)
    dd.close()
    md.close()
