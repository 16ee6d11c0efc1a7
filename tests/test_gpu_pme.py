"""GPU tests of smooth particle-mesh Ewald on charged engines (emdee_md_set_pme): the fixed-point charge mesh, the library's own
3-D FFT, the spectrum multiply and the gather, behind the real-space terms of emdee_md_set_ewald.  The yardstick of the Coulomb
part is tests/helpers/pme_ref.py (numpy fp64, itself checked on the CPU in tests/test_pme_host.py); the LJ part is
tests/helpers/ortho_ref.py or the oracle, the bonded part tests/helpers/bonded_ref.py, as in tests/test_gpu_ewald.py, whose helpers
these tests import.

Tolerances.  An engine and the reference sum the same truncated series on the same mesh, so neither the truncation nor the mesh
error enters a comparison: fp64 outputs agree to 1e-9 of the largest entry and fp32 outputs to 1e-4, the tolerances of the Ewald
tests.  The fixed-point mesh adds at most half a quantum of 2^-60 sum |q| per contribution, far below either."""
import ctypes as C

import numpy as np
import pytest

from .helpers import ewald_ref as er
from .helpers import ortho_ref as orf
from .helpers import pme_ref as pr
from .test_gpu_bonded import _box, _chains, _outputs
from .test_gpu_coulomb import _water
from .test_gpu_dd_pairs import _build, _lj14scale
from .test_gpu_ewald import (ALPHA, ERR_INVALID, ERR_STATE, KMAX, RC_BOX, RS_BOX, SKIN_BOX, _bits, _chain_engine, _close, _compare,
                             _engine, _forces, _lj_box, _no_lj)
from .test_pme_host import MEASURED

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

GRID = (8, 16, 32)                                                     # small and unequal: every stencil wraps, the shortest FFT


# ---------------------------------------------------------------- 1. random charges with LJ
_REFERENCES = {}


def _lj_reference(E, single, grid, order):
    """(pos, L, q, atoms, (f, e, w, t)) of the 300-charge box with LJ: ortho_ref + pme_ref, computed once per mesh and shared"""
    key = (single, tuple(grid), order)
    if key not in _REFERENCES:
        pos, L, q, eps, sigma = _lj_box()
        if single:
            pos = pos.astype(np.float32).astype(np.float64)
        atoms = E.lennard_jones_atoms(eps, sigma)
        lj = orf.nonbonded(pos, (0, 0, 0), L, (1, 1, 1), RC_BOX, RS_BOX, atoms)
        pm = pr.pme(pos, L, q, 1.0, ALPHA, grid, order, RC_BOX)
        _REFERENCES[key] = (pos, L, q, atoms, tuple(lj[k] + c for k, c in zip("fewt", pm)))
    return _REFERENCES[key]


def _lj_case(E, monkeypatch, path, dtype, grid, order):
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    single = dtype == torch.float32
    pos, L, q, atoms, ref = _lj_reference(E, single, grid, order)
    md = _engine(E, pos, L, atoms, RC_BOX, RS_BOX, SKIN_BOX, dtype=dtype)
    md.set_coulomb_(q, 1.0)
    md.set_pme_(ALPHA, grid, order)
    _compare(md, ref, 1e-4 if single else 1e-9)
    md.close()


@pytest.mark.parametrize("order", [4, 6])
@pytest.mark.parametrize("path,dtype", [("brick", torch.float64), ("direct", torch.float64), ("brick", torch.float32),
                                        ("direct", torch.float32)])
def test_random_charges_with_lj_match_the_references(emdee, monkeypatch, path, dtype, order):
    _lj_case(emdee, monkeypatch, path, dtype, GRID, order)


def test_random_charges_on_a_mesh_with_the_long_axis_first(emdee, monkeypatch):
    _lj_case(emdee, monkeypatch, "brick", torch.float64, (64, 32, 16), 4)


@pytest.mark.parametrize("grid", [(128, 8, 8), (8, 8, 256)])
def test_random_charges_on_the_longest_axes(emdee, monkeypatch, grid):
    # 128 and 256 points: 16 and 8 lines per workgroup of the transform, the fewest; strided (x) and contiguous (z)
    _lj_case(emdee, monkeypatch, "brick", torch.float64, grid, 4)


# ---------------------------------------------------------------- 2. a box with a net charge
def test_net_charge_energy_has_the_background_and_the_virial_is_the_volume_derivative(emdee):
    # The mesh: order 6 on 32^3, where the mesh energy is within a relative 4e-5 of the exact one, so that E(mu) = E / mu holds
    # well enough for the truncation error h^2 |E''') / 6 = h^2 |E| of the central difference (tests/test_pme_host.py
    # test_reference_tensor_sums_to_the_volume_derivative_of_its_energy has the reasoning; tests/test_gpu_ewald.py test 3 the bound).
    E = emdee
    grid, order = (32, 32, 32), 6
    pos, L, q = er.random_charges(min_sep=0.8, total=15.0)
    md = _engine(E, pos, L, _no_lj(E, pos.shape[0]), RC_BOX, RS_BOX, SKIN_BOX)
    md.set_coulomb_(q, 1.0)
    md.set_pme_(ALPHA, grid, order)
    ref = pr.pme(pos, L, q, 1.0, ALPHA, grid, order, RC_BOX)
    background = -np.pi * q.sum() ** 2 / (2 * float(np.prod(L)) * ALPHA ** 2)
    ep, _, w = md.totals()
    print("energy %.12g reference %.12g (background %.6g); virial %.12g reference %.12g" % (ep, ref[1].sum(), background, w, ref[2].sum()))
    assert abs(ep - ref[1].sum()) <= 1e-9 * abs(ref[1].sum()) and abs(background) > 1e-3 * abs(ep)
    assert abs(w - ref[2].sum()) <= 1e-9 * abs(ref[2].sum())
    h = 1e-4
    md.scale_box_(1.0 + h)
    e_plus = md.totals()[0]
    md.scale_box_((1.0 - h) / (1.0 + h))
    e_minus = md.totals()[0]
    dE = (e_plus - e_minus) / (2 * h)
    print("virial %.12g, -dE/dmu %.12g, difference %.3e, bound %.3e" % (w, -dE, abs(w + dE), (h * h + 1e-9) * abs(ep)))
    assert abs(w + dE) <= (h * h + 1e-9) * abs(ep)
    md.close()


# ---------------------------------------------------------------- 3. exclusions and 1-4 pairs
@pytest.mark.parametrize("path,dtype", [("brick", torch.float64), ("direct", torch.float64), ("brick", torch.float32)])
def test_chains_correct_their_excluded_pairs_and_scale_their_14_pairs(emdee, monkeypatch, path, dtype):
    E = emdee
    if path == "direct":
        monkeypatch.setenv("EMDEE_PATH", "direct")
    pos, vel, eps, sigma, L = _box(E, ncell=4)
    N = pos.shape[0]
    if dtype == torch.float32:
        pos = pos.astype(np.float32).astype(np.float64)
    terms, excl, p14 = _chains(N)
    s14, c14 = _lj14scale(E), 0.8333
    q = np.tile([0.6, -0.3, -0.5, 0.2], N // 4)
    rc, rs, skin = 2.5, 2.0, 0.3
    md = _engine(E, pos, L, E.lennard_jones_atoms(eps, sigma), rc, rs, skin, dtype=dtype)
    md.set_exclusions_(excl)
    md.set_pairs14_(p14, s14)
    for kind, a, p in terms:
        md.set_bonded_(kind, a, p)
    tol = 1e-9 if dtype == torch.float64 else 1e-4
    uncharged = [_forces(md)] + _outputs(md)
    alpha, grid, order = 1.4, (16, 8, 32), 4
    md.set_coulomb_(q, 1.0, 5.0, c14)
    md.set_pme_(alpha, grid, order)
    charged = [_forces(md)] + _outputs(md)
    pm = pr.pme(pos, L, q, 1.0, alpha, grid, order, rc, excl=excl, p14=p14, s14=c14)
    for k, what in ((0, "force-only"), (1, "forces"), (2, "energies"), (3, "virials"), (4, "tensors")):
        want = pm[max(k - 1, 0)]
        err = np.abs((charged[k] - uncharged[k]) - want).max() / max(np.abs(want).max(), np.abs(charged[k]).max())
        print("%s: Coulomb part, max error / max entry = %.3e" % (what, err))
        assert err <= tol, what
    md.close()


# ---------------------------------------------------------------- 4. water
WATER_GRID, WATER_ORDER = (32, 32, 32), 4


def _water_pme(E):
    w, pos, terms = _water(E)
    rc = 0.9
    return w, pos, terms, rc, 3.5 / rc


def _water_engine(E, w, pos, terms, rc, alpha, vel=None):
    md = _engine(E, pos, w["L"], w["atoms"], rc, 0.8, 0.1, vel=vel, inv_mass=w["inv_mass"])
    md.set_exclusions_(w["exclusions"])
    for kind, a, p in terms:
        md.set_bonded_(kind, a, p)
    return md


def test_water_matches_the_references(emdee):
    E = emdee
    w, pos, terms, rc, alpha = _water_pme(E)
    md = _water_engine(E, w, pos, terms, rc, alpha)
    uncharged = _outputs(md)
    md.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
    md.set_pme_(alpha, WATER_GRID, WATER_ORDER)
    charged = _outputs(md)
    pm = pr.pme(pos, w["L"], w["charges"], E.COULOMB_K_KJ_NM, alpha, WATER_GRID, WATER_ORDER, rc, excl=w["exclusions"])
    for got, want, what in zip([a - b for a, b in zip(charged[:4], uncharged[:4])], pm, ("forces", "energies", "virials", "tensors")):
        _close(got, want, 1e-9, "Coulomb part of the " + what)
    md.close()


def test_pme_water_nve_energy_error_scales_as_dt_squared(emdee):
    E = emdee
    w, _, terms, rc, alpha = _water_pme(E)
    pos = _water(E, jitter=0.0)[1]
    N = pos.shape[0]
    m = 1.0 / w["inv_mass"]
    vel = np.random.default_rng(11).standard_normal((N, 3)) * np.sqrt(2.0 / m)[:, None]
    vel -= (m[:, None] * vel).sum(axis=0) / m.sum()
    rms = []
    for dt, every in ((0.0004, 1), (0.0002, 2)):
        md = _water_engine(E, w, pos, terms, rc, alpha, vel=vel)
        md.set_coulomb_(w["charges"], E.COULOMB_K_KJ_NM, np.inf)
        md.set_pme_(alpha, WATER_GRID, WATER_ORDER)
        tot = []
        for _ in range(100):
            md.step_(every, dt)
            ep, ek, _ = md.totals()
            tot.append(ep + ek)
        rms.append(np.std(tot))
        f = _forces(md)
        # (the mesh breaks translation invariance: its forces do not sum to zero, so momentum is not asserted)
        print("dt %g: net force %s against the largest force %.3e" % (dt, f.sum(axis=0), np.abs(f).max()))
        md.close()
    print("rms of the total energy", rms)
    assert 3.0 <= rms[0] / rms[1] <= 5.0, rms


# ---------------------------------------------------------------- 5. convergence on the device
def test_fine_mesh_forces_agree_with_the_direct_sum_of_the_same_engine(emdee):
    E = emdee
    pos, L, q = er.random_charges()
    md = _engine(E, pos, L, _no_lj(E, pos.shape[0]), RC_BOX, RS_BOX, SKIN_BOX)
    md.set_coulomb_(q, 1.0)
    md.set_ewald_(ALPHA, KMAX)
    direct = _forces(md)
    md.set_pme_(ALPHA, (64, 64, 64), 6)
    mesh = _forces(md)
    err = np.sqrt(((mesh - direct) ** 2).mean()) / np.sqrt((direct ** 2).mean())
    print("order 6, 64^3: rms force error / rms force = %.4e (CPU reference: %.3e)" % (err, MEASURED[(6, 64)]))
    assert err <= 2.0 * MEASURED[(6, 64)]
    md.close()


# ---------------------------------------------------------------- 6. bits
@pytest.mark.parametrize("dtype", [torch.float64, torch.float32])
def test_runs_repeat_and_switching_restores_the_other_settings_bits(emdee, dtype):
    E = emdee
    never, toggled, again, ewald, both = (_chain_engine(E, dtype) for _ in range(5))
    grid, order = (16, 8, 32), 4
    toggled.set_pme_(1.4, grid, order)
    again.set_pme_(1.4, grid, order)
    ewald.set_ewald_(1.4, 9)
    both.set_pme_(1.4, grid, order)
    both.set_ewald_(1.4, 9)
    for md in (never, toggled, again, ewald, both):
        md.step_(10, 0.002)
    # (one _bits per engine: a second call would return the energies of the tensor pass, which the first call leaves current)
    rf, pm, pm2, ew, ew2 = (_bits(md) for md in (never, toggled, again, ewald, both))
    for a, b in zip(pm, pm2):
        assert torch.equal(a, b)                                       # two identical PME runs: the same bits
    assert not torch.equal(pm[2], rf[2])                               # ... not the reaction field's
    assert not torch.equal(pm[2], ew[2])                               # ... and not the direct sum's
    for a, b in zip(ew, ew2):
        assert torch.equal(a, b)                                       # set_pme_ then set_ewald_: the direct sum alone
    # back to the reaction field from the same state: the engine that never left it gives the same bits
    st = never.state()
    toggled.set_pme_(0.0)
    dev = torch.device("cuda", 0)
    pos, vel, eps, sigma, L = _box(E, ncell=4)
    atoms = E.cu(E.lennard_jones_atoms(eps, sigma), dev)
    for md in (never, toggled):
        md.set_state_(st["positions"].clone(), st["velocities"].clone(), atoms)
        md.step_(10, 0.002)
    for a, b in zip(_bits(never), _bits(toggled)):
        assert torch.equal(a, b)
    for md in (never, toggled, again, ewald, both):
        md.close()


def test_scale_box_keeps_the_setting_and_equals_a_fresh_engine_on_the_scaled_state(emdee):
    E = emdee
    pos, L, q, eps, sigma = _lj_box(total=1.0)
    atoms = E.lennard_jones_atoms(eps, sigma)
    md = _engine(E, pos, L, atoms, RC_BOX, RS_BOX, SKIN_BOX)
    md.set_coulomb_(q, 1.0)
    md.set_pme_(ALPHA, GRID, 6)
    md.scale_box_([1.02, 1.01, 1.03])
    scaled = _outputs(md)
    lo, lengths = md.box()
    x = md.state()["positions"].cpu().numpy()
    fresh = _engine(E, x, lengths, atoms, RC_BOX, RS_BOX, SKIN_BOX)
    fresh.set_coulomb_(q, 1.0)
    fresh.set_pme_(ALPHA, GRID, 6)
    for a, b, what in zip(scaled, _outputs(fresh), ("forces", "energies", "virials", "tensors", "box tensor")):
        _close(a, b, 1e-12, what)
    ref = pr.pme(x, np.array(lengths), q, 1.0, ALPHA, GRID, 6, RC_BOX)
    lj = orf.nonbonded(x, (0, 0, 0), np.array(lengths), (1, 1, 1), RC_BOX, RS_BOX, atoms)
    _close(scaled[0], ref[0] + lj["f"], 1e-9, "forces on the scaled box against the references")
    for e in (md, fresh):
        e.close()


def test_the_mesh_pass_is_timed_under_index_8(emdee):
    E = emdee
    pos, L, q = er.random_charges(min_sep=0.8)
    md = _engine(E, pos, L, _no_lj(E, pos.shape[0]), RC_BOX, RS_BOX, SKIN_BOX)
    md.set_coulomb_(q, 1.0)
    md.set_pme_(ALPHA, GRID, 4)
    md.profile_(True)
    for _ in range(3):
        md.forces_()
    ms, launches = md.kernel_time("ewald_reciprocal")
    print("reciprocal pass: %.4f ms over %d launches" % (ms, launches))
    assert launches == 3 and ms > 0.0
    md.close()


# ---------------------------------------------------------------- 7. refusals
def test_invalid_and_out_of_state_calls_are_refused_and_keep_the_setting(emdee):
    E = emdee
    dev = torch.device("cuda", 0)
    pos, L, q = er.random_charges(min_sep=0.8)
    n = pos.shape[0]
    atoms = _no_lj(E, n)
    md = _engine(E, pos, L, atoms, RC_BOX, RS_BOX, SKIN_BOX)
    before = _forces(md)
    with pytest.raises(E.EmDeeError) as err:                           # no charges yet
        md.set_pme_(ALPHA, GRID, 4)
    assert err.value.code == ERR_STATE
    md.forces_()
    assert np.array_equal(_forces(md), before)
    md.set_coulomb_(q, 1.0)
    rf = _forces(md)
    md.set_pme_(ALPHA, GRID, 4)
    f0 = _forces(md)
    assert np.abs(f0 - rf).max() > 1e-3 * np.abs(f0).max()
    bad = [(-1.0, GRID, 4), (np.nan, GRID, 4), (np.inf, GRID, 4), (0.9 / RC_BOX, GRID, 4), (ALPHA, None, 4), (ALPHA, (4, 16, 32), 4),
           (ALPHA, (8, 512, 32), 4), (ALPHA, (8, 16, 24), 4), (ALPHA, (8, 16, -32), 4), (ALPHA, (8, 16, 0), 4), (ALPHA, GRID, 5),
           (ALPHA, GRID, 8), (ALPHA, GRID, 2), (ALPHA, GRID, 0)]
    for alpha, grid, order in bad:
        with pytest.raises(E.EmDeeError) as err:
            md.set_pme_(alpha, grid, order)
        assert err.value.code == ERR_INVALID, (alpha, grid, order)
        md.forces_()
        assert np.array_equal(_forces(md), f0), (alpha, grid, order)   # the previous setting is in force
    # the setting survives new charges and a state with the same atom count; clearing the charges switches it off
    md.set_coulomb_(q, 1.0)
    assert np.array_equal(_forces(md), f0)
    md.set_state_(E.cu(pos, dev), E.cu(np.zeros((n, 3)), dev), E.cu(atoms, dev))
    assert np.array_equal(_forces(md), f0)
    md.set_coulomb_(None, 1.0)
    md.set_coulomb_(q, 1.0)
    assert np.array_equal(_forces(md), rf)
    md.set_pme_(ALPHA, GRID, 4)
    md.set_ewald_(0.0)                                                 # alpha = 0 through either call: the reaction field
    assert np.array_equal(_forces(md), rf)
    md.set_pme_(ALPHA, GRID, 4)
    md.set_pme_(0.0)                                                   # (alpha = 0: grid and order are not looked at)
    assert np.array_equal(_forces(md), rf)
    md.set_pme_(0.0, (3, 3, 3), 7)
    assert np.array_equal(_forces(md), rf)
    md.close()
    # before emdee_md_set_state
    h = C.c_void_p()
    model = E.LennardJonesModel(RC_BOX, RS_BOX)
    E._lib.call("emdee_md_create", E.device.context_for(dev).handle, (C.c_double * 3)(0, 0, 0), (C.c_double * 3)(*L), (C.c_int32 * 3)(1, 1, 1),
                E._lib.model_c(model), SKIN_BOX, E.device.precision_of(E.cu(pos, dev)), C.byref(h))
    with pytest.raises(E.EmDeeError) as err:
        E._lib.call("emdee_md_set_pme", h, ALPHA, (C.c_int32 * 3)(*GRID), 4)
    assert err.value.code == ERR_STATE
    E._lib.call("emdee_md_destroy", h)
    # a box that is not periodic in all three dimensions
    inner = np.clip(pos, 0.5, np.array(L) - 0.5)
    md = _engine(E, inner, L, atoms, RC_BOX, RS_BOX, SKIN_BOX, periodic=(1, 1, 0))
    md.set_coulomb_(q, 1.0)
    before = _forces(md)
    with pytest.raises(E.EmDeeError) as err:
        md.set_pme_(ALPHA, GRID, 4)
    assert err.value.code == ERR_STATE
    md.forces_()
    assert np.array_equal(_forces(md), before)
    md.close()
    # an integrator with ghosts
    md = _engine(E, pos, L, atoms, RC_BOX, RS_BOX, SKIN_BOX, n_ghost=10)
    before = _forces(md)
    with pytest.raises(E.EmDeeError) as err:
        md.set_pme_(ALPHA, GRID, 4)
    assert err.value.code == ERR_STATE
    md.forces_()
    assert np.array_equal(_forces(md), before)
    md.close()
    # an integrator lent by a decomposition
    bpos, bvel, eps, sigma, bL = _box(E, ncell=6)
    dd = _build(E, 2, bpos, bvel, E.lennard_jones_atoms(eps, sigma), bL)
    dd.set_coulomb_(np.where(np.arange(bpos.shape[0]) % 2 == 0, 0.5, -0.5), 1.0)
    before = dd.engine(0).state(positions=False, velocities=False)["forces"].clone()
    with pytest.raises(E.EmDeeError) as err:
        dd.engine(0).set_pme_(1.4, (16, 16, 16), 4)
    assert err.value.code == ERR_STATE
    assert torch.equal(dd.engine(0).state(positions=False, velocities=False)["forces"], before)
    dd.close()
