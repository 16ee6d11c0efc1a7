"""GPU tests of the Ewald sum of charged engines (emdee_md_set_ewald): erfc pair terms in the pair loops, the correction of
excluded and 1-4 pairs, the direct reciprocal-space sum.  The yardstick of the Coulomb part is tests/helpers/ewald_ref.py (numpy /
scipy fp64, itself checked on the CPU in tests/test_ewald_host.py); the LJ part is tests/helpers/ortho_ref.py (boxes with three
different sides) or the oracle, the bonded part tests/helpers/bonded_ref.py.

Tolerances.  An engine and the reference sum the same truncated series, so the truncation does not enter a comparison: fp64
outputs agree to 1e-9 of the largest entry and fp32 outputs to 1e-4, the tolerances of the reaction-field tests (a few hundred
pair terms of relative rounding 1e-15 / 1e-7 each, and the fast reciprocal and reciprocal square root of the pair loops)."""
import ctypes as C

import numpy as np
import pytest

from .helpers import coulomb_ref as cr
from .helpers import ewald_ref as er
from .helpers import ortho_ref as orf
from .test_gpu_bonded import _box, _chains, _outputs, _reference
from .test_gpu_coulomb import _water
from .test_gpu_dd_pairs import _build, _lj14scale

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ERR_INVALID, ERR_STATE = -1, -6
BOX, RC_BOX, RS_BOX, SKIN_BOX = (7.0, 8.0, 9.5), 3.3, 2.8, 0.15    # the 300-charge box: rc + skin just under L_x / 2
ALPHA, KMAX = 1.5, (20, 22, 26)


def _engine(E, pos, L, atoms, rc, rs, skin, dtype=torch.float64, vel=None, inv_mass=None, periodic=None, n_ghost=0):
    dev = torch.device("cuda", 0)
    ndt = np.float64 if dtype == torch.float64 else np.float32
    L = np.broadcast_to(np.asarray(L, dtype=np.float64), (3,))
    vel = np.zeros((pos.shape[0] - n_ghost, 3)) if vel is None else vel
    im = None if inv_mass is None else E.cu(inv_mass.astype(ndt), dev)
    return E.VelocityVerlet(E.cu(pos.astype(ndt), dev), E.cu(vel.astype(ndt), dev), float(L[0]), E.LennardJonesModel(rc, rs),
                            E.cu(atoms, dev), skin=skin, inv_mass=im, lengths=L, periodic=periodic, n_ghost=n_ghost)


def _no_lj(E, n):
    return E.lennard_jones_atoms(0.0, 1.0, n)


def _forces(md):
    return md.state(positions=False, velocities=False)["forces"].cpu().numpy().astype(np.float64)


def _close(got, want, tol, what):
    err = np.abs(got - want).max() / np.abs(want).max()
    print("%s: max error / max entry = %.3e (bound %.0e)" % (what, err, tol))
    assert err <= tol, what


def _compare(md, ref, tol):
    """forces of the force-only kernels, then the five outputs of the observable passes, against ref = (f, e, w, t)"""
    _close(_forces(md), ref[0], tol, "forces (force-only pass)")
    out = _outputs(md)
    for got, want, what in zip(out[:4], ref, ("forces", "energies", "virials", "tensors")):
        _close(got, want, tol, what)
    _close(out[4], ref[3].sum(axis=0), 10 * tol * np.abs(ref[3]).max() / np.abs(ref[3].sum(axis=0)).max(), "box tensor")
    trace = np.abs(out[3][:, :3].sum(axis=1) - out[2]).max() / np.abs(out[2]).max()
    print("trace of the tensor against the virial: %.3e" % trace)
    assert trace <= tol
    return out


# ---------------------------------------------------------------- 1. rock salt
def test_rock_salt_gives_the_madelung_constant_and_no_forces(emdee):
    E = emdee
    pos, L, q = er.rock_salt(8)
    md = _engine(E, pos, L, _no_lj(E, pos.shape[0]), 3.0, 2.5, 0.3)
    md.set_coulomb_(q, 1.0)
    md.set_ewald_(1.5, 18)
    f = _forces(md)
    madelung = -2.0 * md.totals()[0] / pos.shape[0]
    print("Madelung error %.3e, largest force %.3e" % (madelung - er.MADELUNG_NACL, np.abs(f).max()))
    assert abs(madelung - er.MADELUNG_NACL) < 1e-8
    assert np.abs(f).max() < 1e-10                                     # in units of K / r0^2 = 1
    assert np.abs(_outputs(md)[0]).max() < 1e-10                       # ... and from the all-outputs pass
    md.close()


# ---------------------------------------------------------------- 2. random charges with LJ
def _lj_box(total=0.0):
    pos, L, q = er.random_charges(min_sep=0.8, total=total)
    rng = np.random.default_rng(17)
    n = pos.shape[0]
    return pos, L, q, rng.uniform(0.5, 1.0, n), rng.uniform(0.8, 0.95, n)


@pytest.mark.parametrize("path,dtype", [("brick", torch.float64), ("direct", torch.float64), ("brick", torch.float32),
                                        ("direct", torch.float32)])
def test_random_charges_with_lj_match_the_references(emdee, monkeypatch, path, dtype):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    pos, L, q, eps, sigma = _lj_box()
    if dtype == torch.float32:
        pos = pos.astype(np.float32).astype(np.float64)
    atoms = E.lennard_jones_atoms(eps, sigma)
    md = _engine(E, pos, L, atoms, RC_BOX, RS_BOX, SKIN_BOX, dtype=dtype)
    md.set_coulomb_(q, 1.0)
    md.set_ewald_(ALPHA, KMAX)
    lj = orf.nonbonded(pos, (0, 0, 0), L, (1, 1, 1), RC_BOX, RS_BOX, atoms)
    ew = er.ewald(pos, L, q, 1.0, ALPHA, KMAX, RC_BOX)
    ref = tuple(lj[k] + c for k, c in zip("fewt", ew))
    _compare(md, ref, 1e-9 if dtype == torch.float64 else 1e-4)
    md.close()


# ---------------------------------------------------------------- 3. a box with a net charge
def test_net_charge_energy_has_the_background_and_the_virial_is_the_volume_derivative(emdee):
    E = emdee
    pos, L, q = er.random_charges(min_sep=0.8, total=15.0)
    md = _engine(E, pos, L, _no_lj(E, pos.shape[0]), RC_BOX, RS_BOX, SKIN_BOX)
    md.set_coulomb_(q, 1.0)
    md.set_ewald_(ALPHA, KMAX)
    ref = er.ewald(pos, L, q, 1.0, ALPHA, KMAX, RC_BOX)
    V = float(np.prod(L))
    background = -np.pi * q.sum() ** 2 / (2 * V * ALPHA ** 2)
    ep, _, w = md.totals()
    print("energy %.12g reference %.12g (background %.6g); virial %.12g reference %.12g" % (ep, ref[1].sum(), background, w, ref[2].sum()))
    assert abs(ep - ref[1].sum()) <= 1e-9 * abs(ref[1].sum()) and abs(background) > 1e-3 * abs(ep)
    assert abs(w - ref[2].sum()) <= 1e-9 * abs(ref[2].sum())
    _compare(md, ref, 1e-9)
    # W = -dE/dmu at mu = 1, all three sides scaled alike, by the central difference over mu = 1 +- h.  The Coulomb energy of a
    # scaled configuration is E / mu, so E''' = -6 E and the truncation error of the difference is h^2 |E'''| / 6 = h^2 |E|:
    # 1e-8 |E| at h = 1e-4.  Each energy is a sum of 300 fp64 terms good to about 1e-13 |E|, which the division by 2 h turns
    # into another 1e-9 |E|.
    h = 1e-4
    md.scale_box_(1.0 + h)
    e_plus = md.totals()[0]
    md.scale_box_((1.0 - h) / (1.0 + h))
    e_minus = md.totals()[0]
    dE = (e_plus - e_minus) / (2 * h)
    print("virial %.12g, -dE/dmu %.12g, difference %.3e, bound %.3e" % (w, -dE, abs(w + dE), (h * h + 1e-9) * abs(ep)))
    assert abs(w + dE) <= (h * h + 1e-9) * abs(ep)
    md.close()


# ---------------------------------------------------------------- 4. exclusions and 1-4 pairs
@pytest.mark.parametrize("path,dtype", [("brick", torch.float64), ("direct", torch.float64), ("brick", torch.float32)])
def test_chains_correct_their_excluded_pairs_and_scale_their_14_pairs(emdee, oracle, monkeypatch, path, dtype):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    pos, vel, eps, sigma, L = _box(E, ncell=4)                          # 256 atoms, L = 4 cells: rc + skin = 2.8 <= L / 2
    N = pos.shape[0]
    if dtype == torch.float32:
        pos = pos.astype(np.float32).astype(np.float64)
    atoms = E.lennard_jones_atoms(eps, sigma)
    terms, excl, p14 = _chains(N)
    s14, c14 = _lj14scale(E), 0.8333
    q = np.tile([0.6, -0.3, -0.5, 0.2], N // 4)
    rc, rs, skin = 2.5, 2.0, 0.3
    assert rc + skin <= L / 2
    md = _engine(E, pos, L, atoms, rc, rs, skin, dtype=dtype)
    md.set_exclusions_(excl)
    md.set_pairs14_(p14, s14)
    for kind, a, p in terms:
        md.set_bonded_(kind, a, p)
    tol = 1e-9 if dtype == torch.float64 else 1e-4
    uncharged = [_forces(md)] + _outputs(md)
    alpha, kmax = 1.4, 9
    md.set_coulomb_(q, 1.0, 5.0, c14)
    md.set_ewald_(alpha, kmax)
    charged = [_forces(md)] + _outputs(md)
    ew = er.ewald(pos, L, q, 1.0, alpha, kmax, rc, excl=excl, p14=p14, s14=c14)
    for k, what in ((0, "force-only"), (1, "forces"), (2, "energies"), (3, "virials"), (4, "tensors")):
        want = ew[max(k - 1, 0)]
        # (the Coulomb part: what the charges added to the same engine's LJ and bonded terms, relative to the whole)
        err = np.abs((charged[k] - uncharged[k]) - want).max() / max(np.abs(want).max(), np.abs(charged[k]).max())
        print("%s: Coulomb part, max error / max entry = %.3e" % (what, err))
        assert err <= tol, what
    if dtype == torch.float64:                                         # the whole: oracle LJ + bonded_ref + ewald_ref
        (want_f, want_e, want_w), _ = _reference(oracle, pos, L, atoms, excl, p14, s14, terms)
        for got, want in zip(charged[1:4], (want_f + ew[0], want_e + ew[1], want_w + ew[2])):
            assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()
    md.close()


def test_a_struck_pair_beyond_the_list_radius_is_refused_and_named(emdee):
    E = emdee
    pos, L, q = er.random_charges(min_sep=0.8)
    d = pos[None, :, :] - pos[:, None, :]
    d -= L * np.rint(d / L)
    r = np.sqrt((d * d).sum(axis=2))
    i, j = np.argwhere(r > RC_BOX + SKIN_BOX + 0.5)[0]
    near = np.argwhere((r > 0) & (r < 1.5))[:4]
    md = _engine(E, pos, L, _no_lj(E, pos.shape[0]), RC_BOX, RS_BOX, SKIN_BOX)
    md.set_coulomb_(q, 1.0)
    md.set_ewald_(ALPHA, KMAX)
    md.set_exclusions_(near)                                           # pairs inside the list radius: taken
    with pytest.raises(E.EmDeeError) as err:
        md.set_exclusions_(np.concatenate([near, [[i, j]]]))
    assert err.value.code == ERR_STATE
    assert "(%d, %d)" % (min(i, j), max(i, j)) in str(err.value) or "(%d, %d)" % (max(i, j), min(i, j)) in str(err.value), str(err.value)
    with pytest.raises(E.EmDeeError) as err:                           # ... and the engine does not step until the table is replaced
        md.step_(1, 0.001)
    assert err.value.code == ERR_STATE
    md.set_exclusions_(near)
    md.step_(2, 0.001)
    md.close()


# ---------------------------------------------------------------- 5. water
def _water_ewald(E):
    w, pos, terms = _water(E)
    rc = 0.9
    alpha = 3.5 / rc
    return w, pos, terms, rc, alpha, er.kmax_estimate(alpha, w["L"], rc)


def test_water_matches_the_oracle_bonded_and_ewald_references(emdee, oracle):
    E = emdee
    w, pos, terms, rc, alpha, kmax = _water_ewald(E)
    L, atoms, N = w["L"], w["atoms"], pos.shape[0]
    print("water: %d atoms, L = %.4f, alpha = %.4f, kmax = %s" % (N, L, alpha, kmax))
    md = _engine(E, pos, L, atoms, rc, 0.8, 0.1, inv_mass=w["inv_mass"])
    md.set_exclusions_(w["exclusions"])
    for kind, a, p in terms:
        md.set_bonded_(kind, a, p)
    uncharged = _outputs(md)
    md.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
    md.set_ewald_(alpha, kmax)
    charged = _outputs(md)
    ew = er.ewald(pos, L, w["charges"], E.COULOMB_K_KJ_NM, alpha, kmax, rc, excl=w["exclusions"])
    for got, want, what in zip([a - b for a, b in zip(charged[:4], uncharged[:4])], ew, ("forces", "energies", "virials", "tensors")):
        _close(got, want, 1e-9, "Coulomb part of the " + what)
    (want_f, want_e, want_w), _ = _reference(oracle, pos, L, atoms, w["exclusions"], np.zeros((0, 2), dtype=int), 1.0, terms, rc=rc, rs=0.8)
    for got, want in zip(charged[:3], (want_f + ew[0], want_e + ew[1], want_w + ew[2])):
        assert np.abs(got - want).max() <= 1e-6 * np.abs(want).max()   # (the oracle's LJ sum: as the reaction-field water test)
    md.close()


def test_ewald_water_nve_energy_error_scales_as_dt_squared_and_momentum_stays(emdee):
    E = emdee
    w, pos, terms, rc, alpha, kmax = _water_ewald(E)
    pos = _water(E, jitter=0.0)[1]
    L, atoms, N = w["L"], w["atoms"], pos.shape[0]
    m = 1.0 / w["inv_mass"]
    vel = np.random.default_rng(11).standard_normal((N, 3)) * np.sqrt(2.0 / m)[:, None]
    vel -= (m[:, None] * vel).sum(axis=0) / m.sum()
    rms, mom = [], []
    for dt, every in ((0.0004, 1), (0.0002, 2)):
        md = _engine(E, pos, L, atoms, rc, 0.8, 0.1, vel=vel, inv_mass=w["inv_mass"])
        md.set_exclusions_(w["exclusions"])
        for kind, a, p in terms:
            md.set_bonded_(kind, a, p)
        md.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
        md.set_ewald_(alpha, kmax)
        tot = []
        for _ in range(100):
            md.step_(every, dt)
            ep, ek, _ = md.totals()
            tot.append(ep + ek)
        rms.append(np.std(tot))
        v = md.state()["velocities"].cpu().numpy()
        mom.append(np.abs((m[:, None] * v).sum(axis=0)).max() / (m[:, None] * np.abs(v)).sum(axis=0).max())
        md.close()
    print("rms of the total energy", rms, "momentum", mom)
    assert 3.0 <= rms[0] / rms[1] <= 5.0, rms
    assert max(mom) < 1e-10, mom


# ---------------------------------------------------------------- 6. switching
def _chain_engine(E, dtype=torch.float64):
    pos, vel, eps, sigma, L = _box(E, ncell=4)
    N = pos.shape[0]
    terms, excl, p14 = _chains(N)
    md = _engine(E, pos, L, E.lennard_jones_atoms(eps, sigma), 2.5, 2.0, 0.3, dtype=dtype, vel=vel)
    md.set_exclusions_(excl)
    md.set_pairs14_(p14, _lj14scale(E))
    for kind, a, p in terms:
        md.set_bonded_(kind, a, p)
    md.set_coulomb_(np.tile([0.6, -0.3, -0.5, 0.2], N // 4), 1.0, 5.0, 0.8333)
    return md


def _bits(md):
    st = md.state(energies=True, virials=True)
    return [st[k] for k in ("positions", "velocities", "forces", "energies", "virials")] + [md.virial_tensor()]


@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_switching_off_restores_the_reaction_field_bits_and_runs_repeat(emdee, dtype):
    E = emdee
    never, toggled, again = _chain_engine(E, dtype), _chain_engine(E, dtype), _chain_engine(E, dtype)
    toggled.set_ewald_(1.4, 9)
    again.set_ewald_(1.4, 9)
    for md in (never, toggled, again):
        md.step_(10, 0.002)
    ew = [_bits(toggled), _bits(again)]
    for a, b in zip(*ew):
        assert torch.equal(a, b)                                       # two identical Ewald runs: the same bits
    assert not torch.equal(ew[0][2], _bits(never)[2])                  # ... and not the reaction field's
    # back to the reaction field from the same state: the engine that never left it gives the same bits
    st = never.state()
    for md in (toggled, again):
        md.set_ewald_(0.0)
    dev = torch.device("cuda", 0)
    pos, vel, eps, sigma, L = _box(E, ncell=4)
    atoms = E.cu(E.lennard_jones_atoms(eps, sigma), dev)
    for md in (never, toggled):
        md.set_state_(st["positions"].clone(), st["velocities"].clone(), atoms)
        md.step_(10, 0.002)
    for a, b in zip(_bits(never), _bits(toggled)):
        assert torch.equal(a, b)
    for md in (never, toggled, again):
        md.close()


def test_scale_box_keeps_the_setting_and_equals_a_fresh_engine_on_the_scaled_state(emdee):
    E = emdee
    pos, L, q, eps, sigma = _lj_box(total=1.0)
    atoms = E.lennard_jones_atoms(eps, sigma)
    md = _engine(E, pos, L, atoms, RC_BOX, RS_BOX, SKIN_BOX)
    md.set_coulomb_(q, 1.0)
    md.set_ewald_(ALPHA, KMAX)
    md.scale_box_([1.02, 1.01, 1.03])
    scaled = _outputs(md)
    lo, lengths = md.box()
    x = md.state()["positions"].cpu().numpy()
    fresh = _engine(E, x, lengths, atoms, RC_BOX, RS_BOX, SKIN_BOX)
    fresh.set_coulomb_(q, 1.0)
    fresh.set_ewald_(ALPHA, KMAX)
    for a, b, what in zip(scaled, _outputs(fresh), ("forces", "energies", "virials", "tensors", "box tensor")):
        _close(a, b, 1e-12, what)
    ref = er.ewald(x, np.array(lengths), q, 1.0, ALPHA, KMAX, RC_BOX)
    lj = orf.nonbonded(x, (0, 0, 0), np.array(lengths), (1, 1, 1), RC_BOX, RS_BOX, atoms)
    _close(scaled[0], ref[0] + lj["f"], 1e-9, "forces on the scaled box against the references")
    for e in (md, fresh):
        e.close()


# ---------------------------------------------------------------- 7. refusals
def test_invalid_and_out_of_state_calls_are_refused_and_keep_the_setting(emdee):
    E = emdee
    dev = torch.device("cuda", 0)
    pos, L, q = er.random_charges(min_sep=0.8)
    n = pos.shape[0]
    atoms = _no_lj(E, n)
    md = _engine(E, pos, L, atoms, RC_BOX, RS_BOX, SKIN_BOX)
    with pytest.raises(E.EmDeeError) as err:                           # no charges yet
        md.set_ewald_(ALPHA, KMAX)
    assert err.value.code == ERR_STATE
    md.set_coulomb_(q, 1.0)
    rf = _forces(md)
    md.set_ewald_(ALPHA, KMAX)
    f0 = _forces(md)
    assert np.abs(f0 - rf).max() > 1e-3 * np.abs(f0).max()
    bad = [(-1.0, KMAX), (np.nan, KMAX), (np.inf, KMAX), (ALPHA, None), (ALPHA, (0, 22, 26)), (ALPHA, (20, 65, 26)), (ALPHA, (20, 22, -1)),
           (0.9 / RC_BOX, KMAX)]
    for alpha, kmax in bad:
        with pytest.raises(E.EmDeeError) as err:
            md.set_ewald_(alpha, kmax)
        assert err.value.code == ERR_INVALID, (alpha, kmax)
        md.forces_()
        assert np.array_equal(_forces(md), f0), (alpha, kmax)         # the previous setting is in force
    # the setting survives new charges and a state with the same atom count; clearing the charges switches it off
    md.set_coulomb_(q, 1.0)
    assert np.array_equal(_forces(md), f0)
    md.set_state_(E.cu(pos, dev), E.cu(np.zeros((n, 3)), dev), E.cu(atoms, dev))
    assert np.array_equal(_forces(md), f0)
    md.set_coulomb_(None, 1.0)
    md.set_coulomb_(q, 1.0)
    assert np.array_equal(_forces(md), rf)
    md.set_ewald_(0.0)                                                 # (alpha = 0: kmax is not looked at)
    assert np.array_equal(_forces(md), rf)
    md.close()
    # before emdee_md_set_state
    h = C.c_void_p()
    model = E.LennardJonesModel(RC_BOX, RS_BOX)
    E._lib.call("emdee_md_create", E.device.context_for(dev).handle, (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(*L), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(model), SKIN_BOX, E.device.precision_of(E.cu(pos, dev)), C.byref(h))
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_set_ewald", h, ALPHA, (C.c_int32 * 3)(*KMAX))
    assert err.value.code == ERR_STATE
    E._lib.call("emdee_md_destroy", h)
    # a box that is not periodic in all three dimensions
    inner = np.clip(pos, 0.5, np.array(L) - 0.5)
    md = _engine(E, inner, L, atoms, RC_BOX, RS_BOX, SKIN_BOX, periodic=(1, 1, 0))
    md.set_coulomb_(q, 1.0)
    with pytest.raises(E.EmDeeError) as err:
        md.set_ewald_(ALPHA, KMAX)
    assert err.value.code == ERR_STATE
    md.close()
    # an integrator with ghosts
    md = _engine(E, pos, L, atoms, RC_BOX, RS_BOX, SKIN_BOX, n_ghost=10)
    with pytest.raises(E.EmDeeError) as err:
        md.set_ewald_(ALPHA, KMAX)
    assert err.value.code == ERR_STATE
    md.close()
    # an integrator lent by a decomposition
    bpos, bvel, eps, sigma, bL = _box(E, ncell=6)
    dd = _build(E, 2, bpos, bvel, E.lennard_jones_atoms(eps, sigma), bL)
    dd.set_coulomb_(np.where(np.arange(bpos.shape[0]) % 2 == 0, 0.5, -0.5), 1.0)
    with pytest.raises(E.EmDeeError) as err:
        dd.engine(0).set_ewald_(1.4, 9)
    assert err.value.code == ERR_STATE
    dd.close()
