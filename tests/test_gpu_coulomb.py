"""GPU tests of the reaction-field Coulomb terms (emdee_md_set_coulomb / emdee_dd_set_coulomb).  The yardstick of the Coulomb
part is the numpy restatement tests/helpers/coulomb_ref.py: the charged outputs minus the uncharged ones of the same engine.  The
LJ and bonded parts keep theirs (the oracle, tests/helpers/bonded_ref.py), through tests/test_gpu_bonded.py's constructions."""
import numpy as np
import pytest

from .helpers import bonded_ref as br
from .helpers import coulomb_ref as cr
from .test_gpu_bonded import _box, _chains, _md, _outputs, _reference
from .test_gpu_dd_pairs import _build, _compare, _gather, _global_box, _lj14scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RC, RS, DT = 2.5, 2.0, 0.005
ERR_INVALID, ERR_STATE = -1, -6
K_SIGMA = 1.0                                                   # Coulomb's constant of the sigma-unit boxes


def _alternating(N, q=0.5):
    return q * np.where(np.arange(N) % 2 == 0, 1.0, -1.0)


def _forces_only(md):
    """the force plane as the integrator's force-only kernels left it (no observable query first: that would re-evaluate it
    with the all-outputs kernel)"""
    return md.state(positions=False, velocities=False)["forces"].cpu().numpy().astype(np.float64)


def _check_force_only(f_charged, f_uncharged, ref_f, tol):
    assert np.abs((f_charged - f_uncharged) - ref_f).max() <= tol * np.abs(ref_f).max()


def _check_coulomb_part(charged, uncharged, ref, tol):
    """charged - uncharged against coulomb_ref (f, e, w, t), each relative to its largest entry; and the box tensor sums"""
    for got, want in zip([a - b for a, b in zip(charged[:4], uncharged[:4])], ref):
        assert np.abs(got - want).max() <= tol * np.abs(want).max()
    tsum = ref[3].sum(axis=0)
    assert np.abs((charged[4] - uncharged[4]) - tsum).max() <= tol * np.abs(ref[3]).max() * 10


@pytest.mark.parametrize("eps_rf", [8.0, np.inf])
@pytest.mark.parametrize("path,dtype", [("brick", torch.float64), ("direct", torch.float64), ("brick", torch.float32),
                                        ("direct", torch.float32)])
def test_alternating_charges_on_one_lj_type_match_the_reference(emdee, monkeypatch, path, dtype, eps_rf):
    """A single-species fcc box (it would take the plane kernel without charges) with alternating +-q."""
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    pos, vel, eps, sigma, L = _global_box(E.synthetic, uniform=True, ncell=8)
    N = pos.shape[0]
    if dtype == torch.float32:
        pos = pos.astype(np.float32).astype(np.float64)
    atoms = E.lennard_jones_atoms(eps, sigma)
    q = _alternating(N)
    md = _md(E, pos, vel, atoms, L, dtype=dtype)
    f_unch = _forces_only(md)
    uncharged = _outputs(md)
    md.set_coulomb_(q, K_SIGMA, eps_rf)
    f_ch = _forces_only(md)                                     # the force-only charged instance (rf_force_over_r2)
    charged = _outputs(md)
    ref = cr.coulomb(pos, L, q, K_SIGMA, RC, eps_rf)
    tol = 1e-9 if dtype == torch.float64 else 1e-4
    _check_force_only(f_ch, f_unch, ref[0], tol)
    _check_coulomb_part(charged, uncharged, ref, tol)
    # per-atom tensors: trace = virial, charged as uncharged
    assert np.abs(charged[3][:, :3].sum(axis=1) - charged[2]).max() <= 1e-9 * np.abs(charged[2]).max() * (1 if dtype == torch.float64 else 1e5)
    md.close()


@pytest.mark.parametrize("dtype,ncell,rc,rs,eps_rf", [(torch.float64, 10, 3.0, 2.5, 6.0), (torch.float32, 13, 3.2, 2.7, np.inf)])
def test_long_rows_take_the_charged_instances_of_the_1024_thread_variant(emdee, monkeypatch, capfd, dtype, ncell, rc, rs, eps_rf):
    """Long cutoffs: the charged tile (records + charge plane) is over half a CU's LDS and still fits a whole one, so the plan
    takes variant 8 (1024 threads, 8 lanes per atom).  (The fp32 box has pairs within 1e-6 of rc, inside the rounding of fp32
    positions: the cutoff test may go either way there, so it is checked at eps_rf = inf, where the force is continuous at rc.)"""
    E = emdee
    pos, vel, eps, sigma, L = _global_box(E.synthetic, uniform=True, ncell=ncell)
    N = pos.shape[0]
    if dtype == torch.float32:
        pos = pos.astype(np.float32).astype(np.float64)
    atoms = E.lennard_jones_atoms(eps, sigma)
    q = _alternating(N)
    md = _md(E, pos, vel, atoms, L, dtype=dtype, rc=rc, rs=rs)
    f_unch = _forces_only(md)
    uncharged = _outputs(md)
    monkeypatch.setenv("EMDEE_DEBUG_PLAN", "1")
    capfd.readouterr()
    md.set_coulomb_(q, K_SIGMA, eps_rf)
    plans = [l for l in capfd.readouterr().err.splitlines() if l.startswith("emdee plan: charged engine")]
    assert plans and "brick kernels, variant 8" in plans[-1], plans
    f_ch = _forces_only(md)
    charged = _outputs(md)
    ref = cr.coulomb(pos, L, q, K_SIGMA, rc, eps_rf)
    tol = 1e-9 if dtype == torch.float64 else 1e-4
    _check_force_only(f_ch, f_unch, ref[0], tol)
    _check_coulomb_part(charged, uncharged, ref, tol)
    md.close()


@pytest.mark.parametrize("path", ["brick", "direct"])
def test_chains_exclude_and_scale_their_pairs(emdee, oracle, monkeypatch, path):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    pos, vel, eps, sigma, L = _box(E)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    s14, c14 = _lj14scale(E), 0.8333
    q = np.tile([0.6, -0.3, -0.5, 0.2], N // 4)
    md = _md(E, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14, terms=terms)
    f_unch = _forces_only(md)
    uncharged = _outputs(md)
    md.set_coulomb_(q, K_SIGMA, 5.0, c14)
    f_ch = _forces_only(md)                                     # force-only instance + k_pairs14_q
    charged = _outputs(md)
    ref = cr.coulomb(pos, L, q, K_SIGMA, RC, 5.0, excl=excl, p14=p14, s14=c14)
    _check_force_only(f_ch, f_unch, ref[0], 1e-9)
    _check_coulomb_part(charged, uncharged, ref, 1e-9)
    # the whole: oracle LJ (less the excluded and scaled pairs) + bonded_ref + coulomb_ref
    (want_f, want_e, want_w), _ = _reference(oracle, pos, L, atoms, excl, p14, s14, terms)
    want_f, want_e, want_w = want_f + ref[0], want_e + ref[1], want_w + ref[2]
    assert np.abs(charged[0] - want_f).max() <= 1e-6 * np.abs(want_f).max()
    assert np.abs(charged[1] - want_e).max() <= 1e-6 * np.abs(want_e).max()
    assert np.abs(charged[2] - want_w).max() <= 1e-6 * np.abs(want_w).max()
    md.close()


def _water(E, n=8, jitter=0.005):
    w = E.synthetic.water_box(n)
    N = w["positions"].shape[0]
    pos = np.mod(w["positions"] + np.random.default_rng(7).uniform(-jitter, jitter, (N, 3)), w["L"])
    terms = [(br.BOND, w["bonds"], w["bond_params"]), (br.ANGLE, w["angles"], w["angle_params"])]
    return w, pos, terms


def test_water_matches_the_oracle_bonded_and_coulomb_references(emdee, oracle):
    E = emdee
    w, pos, terms = _water(E)
    L, atoms, N = w["L"], w["atoms"], pos.shape[0]
    rc, rs = 0.9, 0.8
    md = _md(E, pos, np.zeros((N, 3)), atoms, L, excl=w["exclusions"], terms=terms, inv_mass=w["inv_mass"], rc=rc, rs=rs, skin=0.1)
    uncharged = _outputs(md)
    md.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
    charged = _outputs(md)
    ref = cr.coulomb(pos, L, w["charges"], E.COULOMB_K_KJ_NM, rc, np.inf, excl=w["exclusions"])
    _check_coulomb_part(charged, uncharged, ref, 1e-9)
    (want_f, want_e, want_w), bref = _reference(oracle, pos, L, atoms, w["exclusions"], np.zeros((0, 2), dtype=int), 1.0, terms,
                                                rc=rc, rs=rs)
    for got, want in zip(charged[:3], (want_f + ref[0], want_e + ref[1], want_w + ref[2])):
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    md.close()


def test_charged_water_nve_energy_error_scales_as_dt_squared_and_momentum_stays(emdee):
    E = emdee
    w, pos, terms = _water(E, jitter=0.0)
    L, atoms, N = w["L"], w["atoms"], pos.shape[0]
    m = 1.0 / w["inv_mass"]
    vel = np.random.default_rng(11).standard_normal((N, 3)) * np.sqrt(2.0 / m)[:, None]     # ~240 K in kJ/mol, g/mol, nm, ps
    vel -= (m[:, None] * vel).sum(axis=0) / m.sum()
    rms, mom = [], []
    for dt, every in ((0.0004, 1), (0.0002, 2)):
        md = _md(E, pos, vel, atoms, L, excl=w["exclusions"], terms=terms, inv_mass=w["inv_mass"], rc=0.9, rs=0.8, skin=0.1)
        md.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
        tot = []
        for _ in range(100):
            md.step_(every, dt)
            ep, ek, _ = md.totals()
            tot.append(ep + ek)
        rms.append(np.std(tot))
        v = md.state()["velocities"].cpu().numpy()
        mom.append(np.abs((m[:, None] * v).sum(axis=0)).max() / (m[:, None] * np.abs(v)).sum(axis=0).max())
        md.close()
    assert 3.0 <= rms[0] / rms[1] <= 5.0, rms
    assert max(mom) < 1e-10, mom


def test_zero_charges_give_the_uncharged_results_and_clearing_restores_the_uncharged_trajectory(emdee):
    E = emdee
    pos, vel, eps, sigma, L = _box(E, ncell=6)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    s14 = _lj14scale(E)
    ref = _md(E, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14, terms=terms)
    zero = _md(E, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14, terms=terms)
    zero.set_coulomb_(np.zeros(N), K_SIGMA, 10.0, 0.5)
    a, b = _outputs(ref), _outputs(zero)
    for x, y in zip(a, b):
        assert np.abs(x - y).max() <= 1e-13 * max(np.abs(x).max(), 1e-300)
    for md in (ref, zero):
        md.close()
    # (fresh engines: an observable query re-evaluates the forces with the all-outputs kernel, whose rounding differs)
    never = _md(E, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14, terms=terms)
    cleared = _md(E, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14, terms=terms)
    cleared.set_coulomb_(_alternating(N), K_SIGMA)
    cleared.set_coulomb_(None, K_SIGMA)
    for md in (never, cleared):
        md.step_(40, DT)
    s0, s1 = never.state(), cleared.state()
    for k in ("positions", "velocities", "forces"):
        assert torch.equal(s0[k], s1[k]), k
    for md in (never, cleared):
        md.close()


def test_invalid_calls_are_refused_and_keep_the_previous_charges(emdee):
    E = emdee
    pos, vel, eps, sigma, L = _box(E, ncell=6)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    md = _md(E, pos, vel, atoms, L)
    q = _alternating(N)
    md.set_coulomb_(q, K_SIGMA, 4.0)
    f0 = md.state()["forces"].cpu().numpy()
    bad_q = q.copy()
    bad_q[5] = np.nan
    bad = [(q[:-1], K_SIGMA, 4.0, 1.0), (bad_q, K_SIGMA, 4.0, 1.0), (q, np.inf, 4.0, 1.0), (q, 0.0, 4.0, 1.0), (q, -1.0, 4.0, 1.0),
           (q, np.nan, 4.0, 1.0), (q, K_SIGMA, 0.5, 1.0), (q, K_SIGMA, np.nan, 1.0), (q, K_SIGMA, 4.0, -0.1), (q, K_SIGMA, 4.0, np.nan),
           (q, K_SIGMA, 4.0, np.inf)]
    for args in bad:
        with pytest.raises(E.EmDeeError) as err:
            md.set_coulomb_(*args)
        assert err.value.code == ERR_INVALID, args[1:]
    with pytest.raises(E.EmDeeError) as err:                         # a NULL array with n > 0, through the C ABI
        E._lib.call("emdee_md_set_coulomb", md._handle, None, N, 1.0, 4.0, 1.0)
    assert err.value.code == ERR_INVALID
    md.forces_()
    assert np.array_equal(md.state()["forces"].cpu().numpy(), f0)
    md.step_(3, DT)
    # a state with another atom count: the next step is refused until the charges are set again or cleared
    keep = N - 4
    md.set_state_(E.cu(pos[:keep], torch.device("cuda", 0)), E.cu(vel[:keep], torch.device("cuda", 0)), E.cu(atoms[:keep], torch.device("cuda", 0)))
    with pytest.raises(E.EmDeeError) as err:
        md.step_(1, DT)
    assert err.value.code == ERR_STATE
    for query in (lambda: md.state(), lambda: md.totals(), lambda: md.virial_tensor()):   # forces never evaluated for this state
        with pytest.raises(E.EmDeeError) as err:
            query()
        assert err.value.code == ERR_STATE
    assert md.state(forces=False)["positions"].shape[0] == keep  # positions and velocities still read
    md.set_coulomb_(q[:keep], K_SIGMA, 4.0)
    md.step_(2, DT)
    md.close()
    dd = _build(E, 2, pos, vel, atoms, L)
    with pytest.raises(E.EmDeeError) as err:
        dd.engine(0).set_coulomb_(q, K_SIGMA)
    assert err.value.code == ERR_STATE
    dd.close()


def test_a_gid_outside_the_charge_table_is_refused_on_every_domain(emdee):
    E = emdee
    pos, vel, eps, sigma, L = _global_box(E.synthetic, ncell=6)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    dd = _build(E, 8, pos, vel, atoms, L)
    with pytest.raises(E.EmDeeError) as err:
        dd.set_coulomb_(_alternating(N - 1), K_SIGMA)
    assert err.value.code == ERR_STATE
    with pytest.raises(E.EmDeeError) as err:
        dd.step_(1, DT)
    assert err.value.code == ERR_STATE
    dd.set_coulomb_(_alternating(N), K_SIGMA)                        # set again: steps
    dd.step_(2, DT)
    dd.close()


@pytest.mark.parametrize("rebuild_every", [0, 5])
def test_eight_domains_of_charged_chains_match_the_undivided_run(emdee, rebuild_every):
    E = emdee
    pos, vel, eps, sigma, L = _box(E)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    s14 = _lj14scale(E)
    q = np.tile([0.6, -0.3, -0.5, 0.2], N // 4)
    dd = _build(E, 8, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14, load=False)
    for kind, a, p in terms:
        dd.set_bonded_(kind, a, p)
    dd.set_coulomb_(q, K_SIGMA, np.inf, 0.8333)
    dd.load_()
    md = _md(E, pos, vel, atoms, L, excl=excl, p14=p14, s14=s14, terms=terms)
    md.set_coulomb_(q, K_SIGMA, np.inf, 0.8333)
    dd.step_(47, DT, rebuild_every)
    dd.step_(53, DT, rebuild_every)
    md.step_(100, DT, rebuild_every)
    _compare(dd, md, 8, N, L)
    dd.close()
    md.close()


def test_set_coulomb_between_steps_takes_effect_on_return(emdee):
    E = emdee
    pos, vel, eps, sigma, L = _box(E)
    N = pos.shape[0]
    atoms = E.lennard_jones_atoms(eps, sigma)
    dd = _build(E, 8, pos, vel, atoms, L)
    md = _md(E, pos, vel, atoms, L)
    dd.step_(20, DT)
    md.step_(20, DT)
    q = _alternating(N)
    dd.set_coulomb_(q, K_SIGMA, 3.0)
    md.set_coulomb_(q, K_SIGMA, 3.0)
    _, _, f, _ = _gather(dd, 8, N)
    fr = md.state()["forces"].cpu().numpy()
    assert np.abs(f - fr).max() <= 1e-9 * np.abs(fr).max()
    assert dd.totals()[0] == pytest.approx(md.totals()[0], rel=1e-10)
    dd.step_(30, DT)
    md.step_(30, DT)
    _compare(dd, md, 8, N, L)
    dd.close()
    md.close()


def _dd_water(E, w, pos, vel, terms, world, rc, rs, skin):
    dev = torch.device("cuda", 0)
    N = pos.shape[0]
    L = w["L"]
    dd = E.DomainDecomposition([L] * 3, E.domain.rank_grid(world), E.LennardJonesModel(rc, rs), skin=skin, dtype=torch.float64,
                               device=dev)
    for r in range(world):
        mine = np.arange(r, N, world)
        dd.set_atoms_(r, E.cu(pos[mine], dev), E.cu(vel[mine], dev), E.cu(w["atoms"][mine], dev),
                      torch.from_numpy(mine.astype(np.int64)).to(dev))
    dd.set_exclusions_(w["exclusions"])
    for kind, a, p in terms:
        dd.set_bonded_(kind, a, p)
    dd.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
    dd.load_()
    return dd


def test_eight_domains_of_a_charged_water_box_match_the_undivided_run(emdee):
    """(unit masses: the decomposition has none of its own)"""
    E = emdee
    w, pos, terms = _water(E, n=8)
    N = pos.shape[0]
    vel = np.random.default_rng(5).standard_normal((N, 3)) * 0.05
    vel -= vel.mean(axis=0)
    rc, rs, skin, dt = 0.9, 0.8, 0.1, 0.0005
    dd = _dd_water(E, w, pos, vel, terms, 8, rc, rs, skin)
    md = _md(E, pos, vel, w["atoms"], w["L"], excl=w["exclusions"], terms=terms, rc=rc, rs=rs, skin=skin)
    md.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
    dd.step_(100, dt)
    md.step_(100, dt)
    _compare(dd, md, 8, N, w["L"])
    dd.close()
    md.close()
