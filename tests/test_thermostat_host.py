"""CPU tests of the scalar rules of the global thermostats (include/emdee_hip.h: emdee_md_set_thermostat): vrescale_alpha2, the
draws, nhc_step and thermostat_update of emdee.jl_amd/csrc/thermostat.hpp through the stand-alone program
tests/c/thermostat_host.cpp, built with the host compiler under ASan and UBSan, against tests/helpers/thermostat_ref.py and
against the distributions the draws and the thermostat are to sample."""
import os
import subprocess

import numpy as np
import pytest

from .conftest import ROOT
from .helpers import thermostat_ref as tr

EPS = float(np.finfo(np.float64).eps)


@pytest.fixture(scope="session")
def thermostat_host(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("thermostat_host") / "thermostat_host")
    cmd = ["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-Wall", "-Werror",
           os.path.join(ROOT, "tests", "c", "thermostat_host.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr

    def run(case):
        r = subprocess.run([exe], input=" ".join(str(t) for t in case) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0 and r.stderr == "", r.stderr[-2000:]       # (a sanitizer report goes to stderr and aborts)
        return r.stdout
    return run


def _numbers(text):
    return np.array([[float(t) for t in line.split()] for line in text.splitlines()])


# ---------------------------------------------------------------- v-rescale: alpha^2
def _alpha2(thermostat_host, rows):
    case = ["alpha2", len(rows)]
    for row in rows:
        case += [repr(float(t)) for t in row]
    out = _numbers(thermostat_host(case))[:, 0]
    assert len(out) == len(rows)
    return out


def test_alpha2_is_the_numpy_formula(thermostat_host):
    """a table of (K, n_dof, c, R1, S), Kbar = n_dof / 2.  alpha^2 = (sqrt(c) + R1 sqrt(q))^2 + q S with q = (1 - c) Kbar / (n_dof
    K) is a sum of positive terms when R1 >= 0; for R1 < 0 the first two cancel, and the bound carries the largest term: 8 eps
    of (c + q (S + R1^2) + 2 |R1| sqrt(c q)) for the handful of roundings of either side."""
    rng = np.random.default_rng(5)
    n = 300
    n_dof = rng.choice([3, 6, 50, 2589, 100000], n).astype(np.float64)
    K = 0.5 * n_dof * 10.0 ** rng.uniform(-1.0, 1.0, n)
    c = np.exp(-10.0 ** rng.uniform(-3.0, 1.0, n))
    R1 = rng.standard_normal(n)
    S = rng.chisquare(n_dof - 1.0)
    rows = np.column_stack([K, n_dof, c, R1, S])
    got = _alpha2(thermostat_host, rows)
    want = np.array([tr.alpha2(k, d, cc, 0.5 * d, r, s) for k, d, cc, r, s in rows])
    q = (1.0 - c) * 0.5 / K
    bound = 8.0 * EPS * (c + q * (S + R1 * R1) + 2.0 * np.abs(R1) * np.sqrt(c * q))
    assert (np.abs(got - want) <= bound).all(), np.abs((got - want) / bound).max()
    assert (got >= 0.0).all() and (np.abs(got - 1.0) > 1e-6).sum() > 250


def test_alpha_is_one_without_coupling_and_without_kinetic_energy(thermostat_host):
    rows = [[12.5, 50, 1.0, 0.7, 44.0], [3.0, 6, 1.0, -2.5, 9.0], [1e-3, 2589, 1.0, 3.0, 2700.0],      # c = 1: exactly 1
            [0.0, 50, 0.9, 0.7, 44.0], [0.0, 6, 0.0, -1.0, 3.0]]                                          # K = 0: 1
    assert (_alpha2(thermostat_host, rows) == 1.0).all()
    assert all(tr.alpha2(k, d, c, 0.5 * d, r, s) == 1.0 for k, d, c, r, s in rows)


# ---------------------------------------------------------------- the draws
def _draws(thermostat_host, seed, first, n, n_dof):
    out = _numbers(thermostat_host(["draws", seed, first, n, n_dof]))
    assert out.shape == (n, 2)
    return out


def test_draws_are_a_function_of_seed_and_step(thermostat_host):
    a = _draws(thermostat_host, 7, 1, 50, 2590)
    assert np.array_equal(a, _draws(thermostat_host, 7, 1, 50, 2590))
    assert np.array_equal(a[10:], _draws(thermostat_host, 7, 11, 40, 2590))                 # (a step's draws do not depend on the steps before)
    assert len(set(a[:, 0])) == 50 and len(set(a[:, 1])) == 50                              # they differ between steps ...
    b = _draws(thermostat_host, 8, 1, 50, 2590)
    assert not (a[:, 0] == b[:, 0]).any() and not (a[:, 1] == b[:, 1]).any()                # ... and between seeds
    assert np.isfinite(a).all() and (a[:, 1] > 0.0).all()
    # R1 does not depend on n_dof; S does
    c = _draws(thermostat_host, 7, 1, 50, 6)
    assert np.array_equal(a[:, 0], c[:, 0]) and not (a[:, 1] == c[:, 1]).any()
    assert (_draws(thermostat_host, 7, 1, 5, 1)[:, 1] == 0.0).all()                         # no degree of freedom left for S


@pytest.mark.parametrize("nu,seed", [(2, 11), (5, 12), (2589, 13)])
def test_draws_have_the_moments_of_a_normal_and_a_chi_squared(thermostat_host, nu, seed):
    """n = 20000 steps: the sample means and variances lie within 5 standard errors of the distributions' own.  The variance of a
    sample variance is (mu4 - sigma^4) / n: 2 / n for N(0,1); for chi-squared with nu degrees of freedom sigma^2 = 2 nu and
    mu4 = 12 nu (nu + 4), so (8 nu^2 + 48 nu) / n."""
    n = 20000
    m1, v1, ms, vs = _numbers(thermostat_host(["moments", seed, n, nu + 1]))[0]
    print("nu = %d: R1 mean %.4f var %.4f; S mean %.3f (nu %d) var %.2f (2 nu %d)" % (nu, m1, v1, ms, nu, vs, 2 * nu))
    assert abs(m1) <= 5.0 * np.sqrt(1.0 / n)
    assert abs(v1 - 1.0) <= 5.0 * np.sqrt(2.0 / n)
    assert abs(ms - nu) <= 5.0 * np.sqrt(2.0 * nu / n)
    assert abs(vs - 2.0 * nu) <= 5.0 * np.sqrt((8.0 * nu * nu + 48.0 * nu) / n)


# ---------------------------------------------------------------- the chain
def _chain(thermostat_host, K, n_dof, kT, tau, Delta, xi, vxi):
    M = len(xi)
    out = thermostat_host(["chain", repr(float(K)), repr(float(n_dof)), repr(float(kT)), repr(float(tau)), repr(float(Delta)), M]
                          + [repr(float(t)) for t in xi] + [repr(float(t)) for t in vxi]).splitlines()
    alpha, energy = [float(t) for t in out[0].split()]
    return alpha, energy, [float(t) for t in out[1].split()], [float(t) for t in out[2].split()]


@pytest.mark.parametrize("M", [1, 3, 8])
def test_chain_at_rest_at_the_target_leaves_the_particles_alone(thermostat_host, M):
    """K = Kbar with every v_xi = 0: G_1 = 0, so v_1 stays 0, alpha = 1 exactly and xi_1 is unchanged; with M = 1 that is the whole
    chain.  The links above the first are not at rest there -- G_k = (Q_{k-1} v_{k-1}^2 - kT) / Q_k = -1 / tau^2 for v_{k-1} = 0
    -- so for M > 1 their xi_k move (by about -Delta^2 / (2 tau^2)) while nothing reaches the particles."""
    n_dof, kT, tau, Delta = 2589.0, 1.3, 0.4, 0.02
    xi0 = [0.3 - 0.1 * k for k in range(M)]
    alpha, energy, xi, vxi = _chain(thermostat_host, 0.5 * n_dof * kT, n_dof, kT, tau, Delta, xi0, [0.0] * M)
    assert alpha == 1.0 and xi[0] == xi0[0] and vxi[0] == 0.0
    if M == 1:
        assert xi == xi0
    else:
        assert all(v < 0.0 for v in vxi[1:])
        assert all(abs((xi[k] - xi0[k]) / (-0.5 * Delta ** 2 / tau ** 2) - 1.0) < 0.1 for k in range(1, M))


@pytest.mark.parametrize("M", [1, 3, 8])
def test_chain_step_is_undone_by_the_step_of_minus_delta(thermostat_host, M):
    """every pass is a palindrome of maps that invert with -Delta: the state returns to rounding (some sixty operations per link,
    every one of relative error eps on numbers of order one: 1e-13 is two hundred of them)"""
    rng = np.random.default_rng(M)
    n_dof, kT, tau, Delta = 50.0, 0.8, 0.3, 0.05
    xi0, v0 = list(rng.uniform(-1.0, 1.0, M)), list(rng.uniform(-1.0, 1.0, M))
    K0 = 1.4 * 0.5 * n_dof * kT
    a1, _, xi1, v1 = _chain(thermostat_host, K0, n_dof, kT, tau, Delta, xi0, v0)
    assert abs(a1 - 1.0) > 1e-3 and max(abs(a - b) for a, b in zip(v1, v0)) > 1e-3
    a2, _, xi2, v2 = _chain(thermostat_host, a1 * a1 * K0, n_dof, kT, tau, -Delta, xi1, v1)
    gap = max([abs(a1 * a2 - 1.0)] + [abs(a - b) for a, b in zip(xi2 + v2, xi0 + v0)])
    print("M = %d: there and back %.2e" % (M, gap))
    assert gap <= 1e-13


@pytest.mark.parametrize("M", [1, 3, 8])
def test_chain_step_is_the_numpy_restatement(thermostat_host, M):
    """ten events in a row, each from the program's own state, against thermostat_ref.nhc_step from the same state: 1e-14 of
    numbers of order one (the exponentials of the two libraries may differ in the last place)"""
    rng = np.random.default_rng(20 + M)
    n_dof, kT, tau, Delta = 2589.0, 1.0, 0.25, 0.02
    xi, v = [0.0] * M, [0.0] * M
    worst = 0.0
    for k in range(10):
        K = 0.5 * n_dof * kT * float(rng.uniform(0.6, 1.6))
        want = tr.nhc_step(K, n_dof, kT, tau, Delta, M, xi, v)
        alpha, energy, xi, v = _chain(thermostat_host, K, n_dof, kT, tau, Delta, xi, v)
        worst = max([worst, abs(alpha - want[0])] + [abs(a - b) for a, b in zip(xi + v, want[1] + want[2])])
        e = tr.nhc_energy(n_dof, kT, tau, M, xi, v)
        assert abs(energy - e) <= 1e-14 * max(abs(e), n_dof * kT)
    assert worst <= 1e-14 and max(abs(t) for t in v) > 1e-2


def test_chain_conserves_its_energy_with_the_particles(thermostat_host):
    """d(E_th)/dt = -dK/dt for the exact flow; the two-pass factorisation is second order, so for a fixed interval the drift of
    K + E_th falls by four when Delta is halved.  (K is only rescaled here: there are no forces.)"""
    n_dof, kT, tau, M = 50.0, 1.0, 0.5, 3
    drift = []
    for n, Delta in ((20, 0.02), (40, 0.01)):
        K, xi, v = 1.5 * 0.5 * n_dof * kT, [0.0] * M, [0.0] * M
        e0 = K
        for _ in range(n):
            alpha, energy, xi, v = _chain(thermostat_host, K, n_dof, kT, tau, Delta, xi, v)
            K *= alpha * alpha
        drift.append(abs(K + energy - e0))
    print("drift of K + E_th over 0.4: %.3e at 0.02, %.3e at 0.01" % tuple(drift))
    assert drift[0] <= 1e-3 * e0 and 3.0 <= drift[0] / drift[1] <= 5.0


# ---------------------------------------------------------------- the ensemble
def test_vrescale_samples_the_canonical_kinetic_energy_of_oscillators(thermostat_host):
    """50 uncoupled oscillators (omega in [1, 2)) under velocity Verlet with an event after every step: K is Gamma distributed
    with mean Kbar = n_dof kT / 2 and variance 2 Kbar^2 / n_dof.  dt = 0.02 keeps the integrator's own error of the velocity
    distribution ((omega dt)^2 / 4 <= 4e-4) an order below the standard errors, which are batch means over 50 batches of 4000
    steps (tau = 0.2: ten steps)."""
    n_dof, kT, dt, tau, steps, batches = 50, 1.0, 0.02, 0.2, 200000, 50
    K = _numbers(thermostat_host(["ensemble", 2024, n_dof, steps, dt, kT, tau]))[:, 0]
    assert K.shape == (steps,)
    Kbar, var = 0.5 * n_dof * kT, 2.0 * (0.5 * n_dof * kT) ** 2 / n_dof
    bm = K.reshape(batches, -1).mean(axis=1)
    se = bm.std(ddof=1) / np.sqrt(batches)
    y = (K - K.mean()) ** 2
    by = y.reshape(batches, -1).mean(axis=1)
    se_v = by.std(ddof=1) / np.sqrt(batches)
    print("K: mean %.4f (Kbar %.1f, se %.4f); variance %.4f (%.1f, se %.4f)" % (K.mean(), Kbar, se, y.mean(), var, se_v))
    assert se < 0.01 * Kbar and se_v < 0.05 * var                       # (the bounds below mean something)
    assert abs(K.mean() - Kbar) <= 5.0 * se
    assert abs(y.mean() - var) <= 5.0 * se_v
