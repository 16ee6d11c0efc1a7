"""numpy fp64 yardstick of the molecular pressure and of scaling by molecular centres of mass (include/emdee_hip.h:
emdee_md_molecular_pressure_tensor, emdee_md_set_molecular_scaling).  Plain numpy; it never calls the library.

mol: (n, 3) ids {apex, a, b} of the rigid molecules; atoms in no molecule count as molecules of one atom.  Positions are
unwrapped as in settle_ref: the three sites of a molecule differ by the molecule's own vectors, no box lengths.

    M = sum_k m_k,  Y = sum_k m_k y_k / M,  V = sum_k m_k v_k / M,  d_k = y_k - Y
    W_mol^ab = W^ab - sum_mol sum_k 1/2 (d_k^a f_k^b + d_k^b f_k^a)
    K_mol^ab = K^ab - sum_mol (sum_k m_k v_k^a v_k^b - M V^a V^b)          order (xx, yy, zz, xy, xz, yz)
    scale: every site of a molecule moves by (mu - 1) (Y - lo), its velocity gains (velocity_scale - 1) V; one-atom molecules
           and the box scale as barostat_ref.scale does
"""
import numpy as np

from . import barostat_ref as bref
from . import settle_ref as sr

COMPONENTS = ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2))


def centres(x, v, mol, mass):
    """(Y, V, M, d): centres of mass, their velocities, molecular masses, and the sites relative to the centres (n, 3 sites, 3).
    Y is formed from the sites relative to the apex, so that d does not lose digits to a far origin."""
    mol = np.asarray(mol, dtype=np.int64).reshape(-1, 3)
    m = np.asarray(mass, dtype=np.float64)[mol]                                # (n, 3)
    M = m.sum(axis=1)
    y, u = np.asarray(x, dtype=np.float64)[mol], np.asarray(v, dtype=np.float64)[mol]   # (n, 3 sites, 3)
    rel = y - y[:, :1]
    c = (m[:, :, None] * rel).sum(axis=1) / M[:, None]
    V = (m[:, :, None] * u).sum(axis=1) / M[:, None]
    return y[:, 0] + c, V, M, rel - c[:, None]


def corrections(x, v, f, mol, mass):
    """(cw, ck), six numbers each: what the atomic sums W and K hold beyond the molecular ones"""
    mol = np.asarray(mol, dtype=np.int64).reshape(-1, 3)
    if mol.shape[0] == 0:
        return np.zeros(6), np.zeros(6)
    _, V, M, d = centres(x, v, mol, mass)
    m = np.asarray(mass, dtype=np.float64)[mol]
    fk, vk = np.asarray(f, dtype=np.float64)[mol], np.asarray(v, dtype=np.float64)[mol]
    cw = np.array([0.5 * (d[:, :, a] * fk[:, :, b] + d[:, :, b] * fk[:, :, a]).sum() for a, b in COMPONENTS])
    ck = np.array([(m * vk[:, :, a] * vk[:, :, b]).sum() - (M * V[:, a] * V[:, b]).sum() for a, b in COMPONENTS])
    return cw, ck


def kinetic_sums(v, mass):
    m, v = np.asarray(mass, dtype=np.float64), np.asarray(v, dtype=np.float64)
    return np.array([(m * v[:, a] * v[:, b]).sum() for a, b in COMPONENTS])


def molecular_sums(x, v, f, tensors, mol, mass):
    """(W_mol, K_mol) from unwrapped positions, velocities, force-field forces and the per-atom virial tensors (N, 6) -- or their
    six sums -- of ortho_ref.total"""
    t = np.asarray(tensors, dtype=np.float64)
    W = t.sum(axis=0) if t.ndim == 2 else t
    cw, ck = corrections(x, v, f, mol, mass)
    return W - cw, kinetic_sums(v, mass) - ck


def pressure_diagonal(W_mol, K_mol, lengths):
    return (np.asarray(K_mol)[:3] + np.asarray(W_mol)[:3]) / float(np.prod(lengths))


def scale(x, v, lo, lengths, mu, mol, mass, velocity_scale=1.0):
    """(positions, velocities, lengths) after the molecular scale"""
    lo, mu = np.asarray(lo, dtype=np.float64), np.broadcast_to(np.asarray(mu, dtype=np.float64), (3,))
    mol = np.asarray(mol, dtype=np.int64).reshape(-1, 3)
    x, v = np.array(x, dtype=np.float64), np.array(v, dtype=np.float64)
    xs, ln = bref.scale(x, lo, lengths, mu)                                    # one-atom molecules, and the box
    vs = velocity_scale * v
    if mol.shape[0]:
        Y, V, _, _ = centres(x, v, mol, mass)
        for k in range(3):
            xs[mol[:, k]] = x[mol[:, k]] + (mu - 1.0) * (Y - lo)
            vs[mol[:, k]] = v[mol[:, k]] + (velocity_scale - 1.0) * V
    return xs, vs, ln


def coupled_constrained_verlet(pos, vel, force, atomic_virial, nsteps, dt, mol, geom, mass, lo, lengths, kind, p_ref, beta, tau_p,
                               every, coupling=bref.ISOTROPIC, temperature=None, xi=None, first_step=0, langevin=None, observe=None):
    """settle_ref.constrained_verlet with a coupling event after stage (e) of every step that brings the count (from
    first_step) to a multiple of `every`: P_mol from that step's forces and velocities, mu (and the velocity scale) from
    barostat_ref.berendsen_mu / crescale_mu, the molecular scale.
    force(x, lengths, k) -> (N, 3): k = 0 at the start, k = s after the position stage of step s (from 1), k = -s after the
    event of step s (scaled positions, new lengths).  atomic_virial(x, lengths, s) -> the six sums W of the atomic virial
    tensors at the positions of step s, before its event.  langevin = (gamma, temperature, normals) as settle_ref;
    observe(s, x, v, lengths): after every step (and its event).  xi(count): the event's N(0, 1) number (C-rescale).
    Returns (x, v, lengths, events), events = [(s, P diagonal, mu, velocity scale)]."""
    x, v = np.array(pos, dtype=np.float64), np.array(vel, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    im = (1.0 / mass)[:, None]
    ln = np.array(lengths, dtype=np.float64)
    f = force(x, ln, 0)
    count, events = int(first_step), []
    for s in range(1, nsteps + 1):
        x0 = x.copy()
        v += 0.5 * dt * im * f
        if langevin is not None:
            gamma, temp, normals = langevin
            c1 = np.exp(-gamma * dt)
            v = c1 * v + np.sqrt(1.0 - c1 * c1) * np.sqrt(temp * im) * normals(s - 1)
        x += dt * v
        xc = sr.shake(x0, x, mol, geom, mass)
        v += (xc - x) / dt
        x = xc
        f = force(x, ln, s)
        v += 0.5 * dt * im * f
        v = sr.rattle(x, v, mol, mass)
        count += 1
        if count % every == 0:
            Wm, Km = molecular_sums(x, v, f, atomic_virial(x, ln, s), mol, mass)
            P = pressure_diagonal(Wm, Km, ln)
            if kind == bref.BERENDSEN:
                mu, vs = bref.berendsen_mu(P, p_ref, beta, tau_p, every * dt, coupling), 1.0
            else:
                assert coupling == bref.ISOTROPIC
                mu, vs = bref.crescale_mu(P, np.ravel(p_ref)[0], np.ravel(beta)[0], tau_p, every * dt, temperature, float(np.prod(ln)),
                                          xi(count))
            x, v, ln = scale(x, v, lo, ln, mu, mol, mass, vs)
            f = force(x, ln, -s)
            events.append((s, P, mu, vs))
        if observe is not None:
            observe(s, x, v, ln)
    return x, v, ln, events
