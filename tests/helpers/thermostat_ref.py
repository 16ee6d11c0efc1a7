"""Host yardstick of the global thermostats (include/emdee_hip.h: emdee_md_set_thermostat).  Plain numpy fp64; it never calls the
library.  The scalar rules are restated from the papers' formulas in the order the header gives them; the integrator is
barostat_ref.coupled_verlet's velocity Verlet with the thermostat's event (e') after every `every`-th step and, when a barostat
is given, its event (f) behind it (barostat_ref's own functions).

    v-rescale     c = exp(-Delta / tau), Kbar = n_dof kT / 2
                  alpha^2 = c + (1 - c) (S + R1^2) Kbar / (n_dof K) + 2 R1 sqrt(c (1 - c) Kbar / (n_dof K)),  E_th -= (alpha^2 - 1) K
    Nose-Hoover   Q_1 = n_dof kT tau^2, Q_k = kT tau^2; two passes, each: sweep k = M .. 1, s = exp(-(Delta / 2) v_1), K <- s^2 K,
                  xi_k += (Delta / 2) v_k, sweep k = 1 .. M; a sweep's line for link k is
                      v_k <- v_k e ; v_k += (Delta / 4) G_k ; v_k <- v_k e,   e = exp(-(Delta / 8) v_{k+1}) (1 for k = M)
                      G_1 = (2 K - n_dof kT) / Q_1,  G_k = (Q_{k-1} v_{k-1}^2 - kT) / Q_k
                  alpha = the product of the two s;  E_th = sum Q_k v_k^2 / 2 + n_dof kT xi_1 + kT sum_{k > 1} xi_k
"""
import numpy as np

from . import barostat_ref as bref

OFF, VRESCALE, NOSE_HOOVER = 0, 1, 2
_CACHE = {}


def alpha2(K, n_dof, c, Kbar, R1, S):
    if not K > 0.0:
        return 1.0
    q = (1.0 - c) * Kbar / (n_dof * K)
    return max(c + q * (S + R1 * R1) + 2.0 * R1 * np.sqrt(c * q), 0.0)


def _kick(v, k, M, K, n_dof, kT, Q, Delta):
    e = np.exp(-0.125 * Delta * v[k + 1]) if k + 1 < M else 1.0
    G = (2.0 * K - n_dof * kT) / Q[0] if k == 0 else (Q[k - 1] * v[k - 1] * v[k - 1] - kT) / Q[k]
    v[k] = (v[k] * e + 0.25 * Delta * G) * e


def nhc_step(K, n_dof, kT, tau, Delta, M, xi, vxi):
    """(alpha, xi, vxi) after one event over Delta; xi and vxi are sequences of length M"""
    xi, v = [float(t) for t in xi], [float(t) for t in vxi]
    Q = [n_dof * kT * tau * tau] + [kT * tau * tau] * (M - 1)
    alpha = 1.0
    for _ in range(2):
        for k in range(M - 1, -1, -1):
            _kick(v, k, M, K, n_dof, kT, Q, Delta)
        s = float(np.exp(-0.5 * Delta * v[0]))
        alpha *= s
        K *= s * s
        for k in range(M):
            xi[k] += 0.5 * Delta * v[k]
        for k in range(M):
            _kick(v, k, M, K, n_dof, kT, Q, Delta)
    return alpha, xi, v


def nhc_energy(n_dof, kT, tau, M, xi, vxi):
    e = 0.0
    for k in range(M):
        Q = (n_dof if k == 0 else 1.0) * kT * tau * tau
        e += 0.5 * Q * vxi[k] * vxi[k] + (n_dof if k == 0 else 1.0) * kT * xi[k]
    return e


def kinetic(vel, inv_mass=None):
    """sum m v^2 / 2; an atom with inv_mass = 0 counts as 0"""
    v2 = (np.asarray(vel, dtype=np.float64) ** 2).sum(axis=1)
    if inv_mass is None:
        return 0.5 * float(v2.sum())
    w = np.asarray(inv_mass, dtype=np.float64)
    m = np.divide(1.0, w, out=np.zeros_like(w), where=w != 0)
    return 0.5 * float((m * v2).sum())


class Thermostat:
    """the scalars of one thermostat; event(K, s) -> alpha updates them.  draws(s) -> (R1, S) of the event completing step s"""

    def __init__(self, kind, kT, tau, every, n_dof, chain=3, draws=None, first_step=0):
        self.kind, self.kT, self.tau, self.every, self.n_dof, self.M = kind, float(kT), float(tau), int(every), int(n_dof), int(chain)
        self.draws, self.step = draws, int(first_step)
        self.xi, self.vxi, self.energy = [0.0] * self.M, [0.0] * self.M, 0.0
        self.events = []                                    # (s, K, alpha)

    def event(self, K, dt):
        Delta = self.every * dt
        if self.kind == VRESCALE:
            R1, S = self.draws(self.step)
            a2 = alpha2(K, self.n_dof, np.exp(-Delta / self.tau), 0.5 * self.n_dof * self.kT, R1, S)
            alpha = float(np.sqrt(a2))
            self.energy -= (a2 - 1.0) * K
        else:
            alpha, self.xi, self.vxi = nhc_step(K, self.n_dof, self.kT, self.tau, Delta, self.M, self.xi, self.vxi)
            self.energy = nhc_energy(self.n_dof, self.kT, self.tau, self.M, self.xi, self.vxi)
        self.events.append((self.step, K, alpha))
        return alpha


def thermostatted_verlet(pos, vel, lo, lengths, total, nsteps, dt, thermo, inv_mass=None, baro=None):
    """Velocity Verlet with the thermostat's event after every step that brings its count to a multiple of `every`, then -- with
    baro = dict(p_ref, beta, tau_p, every, temperature, xi) -- barostat_ref's C-rescale event on the scaled velocities.
    Returns dict(x, v, lengths, conserved): conserved[s] = U + K + E_th after step s (conserved[0]: the start)."""
    x, v = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
    ln = np.array(lengths, dtype=np.float64)
    im = 1.0 if inv_mass is None else np.asarray(inv_mass, dtype=np.float64)[:, None]
    out = total(x, ln)
    conserved = [float(out["e"].sum()) + kinetic(v, inv_mass) + thermo.energy]
    sb = 0
    for _ in range(nsteps):
        v += 0.5 * dt * im * out["f"]
        x += dt * v
        out = total(x, ln)
        v += 0.5 * dt * im * out["f"]
        thermo.step += 1
        if thermo.step % thermo.every == 0:
            v *= thermo.event(kinetic(v, inv_mass), dt)
        sb += 1
        if baro is not None and sb % baro["every"] == 0:
            P = bref.pressure_diagonal(v, out["t"], ln, inv_mass)
            mu, vs = bref.crescale_mu(P, baro["p_ref"], baro["beta"], baro["tau_p"], baro["every"] * dt, baro["temperature"],
                                      float(np.prod(ln)), baro["xi"](sb))
            x, ln = bref.scale(x, lo, ln, mu)
            v *= vs
            out = total(x, ln)
        conserved.append(float(out["e"].sum()) + kinetic(v, inv_mass) + thermo.energy)
    return dict(x=x, v=v, lengths=ln, conserved=np.array(conserved))


def fluid_case(syn, key, make_thermo, nsteps=40, baro=None):
    """thermostatted_verlet on barostat_ref.fluid864, once per key; make_thermo() -> a fresh Thermostat.  Returns the dict of
    thermostatted_verlet with the thermostat under "thermo"."""
    if key not in _CACHE:
        S = bref.fluid864(syn)
        th = make_thermo()
        R = thermostatted_verlet(S["pos"], S["vel"], np.zeros(3), [S["L"]] * 3, bref.field(S["atoms"]), nsteps, bref.DT, th, baro=baro)
        R["thermo"] = th
        _CACHE[key] = R
    return _CACHE[key]
