"""CPU tests of the host yardstick of the Green-Kubo observables (tests/helpers/gk_ref.py) against itself and against the equations
of motion: the heat flux formed from the pairs directly agrees with the form the engine uses, per-atom energies and tensors
(tests/helpers/ortho_ref.py: nonbonded), and on an open box it is the time derivative of sum (k_i + e_i) x_i -- which fixes its sign
and its convention (the half-pair split of energy and virial) without a GPU."""
import numpy as np
import pytest

from .helpers import barostat_ref as bref
from .helpers import gk_ref as gr
from .helpers import ortho_ref as oref

RC, RS = bref.RC, bref.RS
OPEN = [0, 0, 0]
DTS = (0.004, 0.002, 0.001)


@pytest.fixture(scope="module")
def droplet(emdee_synthetic):
    """256 atoms, 4^3 jittered fcc cells at rho* = 0.8, in a box with open walls far away, T* = 0.9, three different masses"""
    syn = emdee_synthetic
    pos, L = syn.fcc_positions(4)
    N = pos.shape[0]
    assert N == 256
    vel = syn.velocities(N, temperature=0.9)
    inv_mass = 1.0 / (1.0 + 0.5 * (np.arange(N) % 3))
    lengths = np.array([L + 40.0] * 3)
    return dict(pos=pos + 20.0, vel=vel, lengths=lengths, lo=np.zeros(3), atoms=bref.lj_atoms(N), inv_mass=inv_mass, N=N)


def _fields(D, pos):
    return oref.nonbonded(pos, D["lo"], D["lengths"], OPEN, RC, RS, D["atoms"])


@pytest.mark.parametrize("periodic", [OPEN, [1, 1, 1]])
def test_pair_form_and_field_form_of_the_heat_flux_agree(droplet, emdee_synthetic, periodic):
    """J = sum (k + e) v + 1/2 sum r_ij (f_ij . v_i) from the pairs, and sum (k + e) v + sum W . v from ortho_ref's per-atom energies
    and tensors: the same number up to the order of summation, on the droplet and on the periodic 864-atom fluid"""
    if all(periodic):
        S = bref.fluid864(emdee_synthetic)
        pos, vel, lengths, lo, atoms, im = S["pos"], S["vel"], np.array([S["L"]] * 3), np.zeros(3), S["atoms"], None
    else:
        D = droplet
        pos, vel, lengths, lo, atoms, im = D["pos"], D["vel"], D["lengths"], D["lo"], D["atoms"], D["inv_mass"]
    out = oref.nonbonded(pos, lo, lengths, periodic, RC, RS, atoms)
    J, A = gr.heat_flux_fields(vel, out["e"], out["t"], im)
    Jp = gr.heat_flux_pairs(pos, vel, lengths, periodic, RC, RS, atoms, im)
    print("J (fields) %r, J (pairs) %r, sum of |addends| %r" % (J, Jp, A))
    assert (np.abs(J - Jp) <= 1e-12 * A).all()
    assert (np.abs(J) > 1e-6 * A).all()                      # (not zero by symmetry: the comparison means something)
    # the virial part matters: without it the two would agree trivially
    conv = gr.heat_addends(vel, out["e"], out["t"], im)[:, :, 0].sum(axis=0)
    assert (np.abs(J - conv) > 1e-3 * np.abs(J)).any()


def test_massless_atoms_carry_no_kinetic_energy(droplet):
    D = droplet
    out = _fields(D, D["pos"])
    im = D["inv_mass"].copy()
    im[::5] = 0.0
    a = gr.heat_addends(D["vel"], out["e"], out["t"], im)
    assert np.array_equal(a[::5, :, 0], out["e"][::5, None] * D["vel"][::5])


def test_heat_flux_is_the_time_derivative_of_the_energy_moment_to_second_order(droplet):
    """On an open box d/dt sum (k_i + e_i) x_i = J.  The centred difference over +-1 velocity-Verlet step (the integrator is time
    reversible: the step back is a step with -dt) differs from J by the second-order terms of both, so halving dt divides the
    discrepancy by four: a factor in [3.5, 4.5] per halving over dt = 0.004, 0.002, 0.001.  A wrong sign, a missing factor 1/2 in the
    virial part or a full-pair split of the energies leave a discrepancy that does not shrink."""
    D = droplet
    force = lambda x: _fields(D, x)["f"]
    out = _fields(D, D["pos"])
    J, A = gr.heat_flux_fields(D["vel"], out["e"], out["t"], D["inv_mass"])
    G = lambda x, v: gr.energy_moment(x, v, D["lengths"], OPEN, RC, RS, D["atoms"], D["inv_mass"])
    gaps = []
    for dt in DTS:
        xp, vp = oref.verlet(D["pos"], D["vel"], force, 1, dt, D["inv_mass"])
        xm, vm = oref.verlet(D["pos"], D["vel"], force, 1, -dt, D["inv_mass"])
        rate = (G(xp, vp) - G(xm, vm)) / (2.0 * dt)
        gaps.append(np.linalg.norm(rate - J))
        print("dt = %.3f: |centred difference - J| = %.4e of |J| = %.4e" % (dt, gaps[-1], np.linalg.norm(J)))
    ratios = [gaps[k] / gaps[k + 1] for k in range(2)]
    print("ratios per halving of dt: %.3f, %.3f" % tuple(ratios))
    assert gaps[0] < 0.1 * np.linalg.norm(J)
    assert all(3.5 <= r <= 4.5 for r in ratios), ratios
    # the convective part alone is not the derivative
    conv = gr.heat_addends(D["vel"], out["e"], out["t"], D["inv_mass"])[:, :, 0].sum(axis=0)
    assert np.linalg.norm(conv - J) > 100 * gaps[-1]


def test_correlate_counts_and_stress_words():
    rng = np.random.default_rng(3)
    A = rng.normal(0.0, 5.0, (13, 9))
    ref = gr.correlate(A, 5)
    assert list(ref["counts"]) == [13, 12, 11, 10, 9]
    assert np.allclose(ref["sums"][0], (A * A).sum(axis=0), rtol=1e-14) and np.allclose(ref["sums"][4], (A[4:] * A[:-4]).sum(axis=0), rtol=1e-14)
    assert np.allclose(ref["totals"], A.sum(axis=0), rtol=1e-14)
    t = rng.normal(0.0, 100.0, 12)
    w = gr.stress_words(t)
    S = t[6:] + t[:6]
    assert np.array_equal(w[:3], S[3:]) and w[3] == 0.5 * (S[0] - S[1]) and w[4] == 0.5 * (S[1] - S[2]) and w[5] == (S[0] + S[1] + S[2]) / 3.0
