"""numpy restatement of the bonded terms (include/emdee_hip.h, emdee_*_set_bonded): harmonic bonds, harmonic angles and
periodic torsions, with the engine's per-atom convention.

Vectors inside a term are chained minimum images along its bonds (d_ij = mi(r_j - r_i), then d_jk, d_kl), so a term that
crosses the periodic boundary is unwrapped.  Every atom of a term receives its own force (-grad U) and an equal share (1/2,
1/3, 1/4) of the term's energy U, of its virial W = sum_a x_a . F_a and of its symmetrised tensor sum_a x_a (x) F_a
(order xx, yy, zz, xy, xz, yz), x_a being the unwrapped positions.  A term at a geometry where the direction of its force is
undefined (a bond of length 0, a straight or folded angle, a torsion with a collinear bond pair) has zero force and a finite
energy: the header's contract."""
import numpy as np

BOND, ANGLE, TORSION = 1, 2, 3
ATOMS = {BOND: 2, ANGLE: 3, TORSION: 4}


def _mi(d, L):
    L = np.asarray(L, dtype=np.float64)
    return d - L * np.round(d / L)


def unwrapped(x, idx, L):
    """positions of one term's atoms, chained along its bonds from its first atom"""
    u = [x[idx[0]].astype(np.float64)]
    for a, b in zip(idx[:-1], idx[1:]):
        u.append(u[-1] + _mi(x[b] - x[a], L))
    return np.array(u)


def term_energy(kind, u, p):
    if kind == BOND:
        r = np.linalg.norm(u[1] - u[0])
        return 0.5 * p[0] * (r - p[1]) ** 2
    if kind == ANGLE:
        a, b = u[0] - u[1], u[2] - u[1]
        th = np.arctan2(np.linalg.norm(np.cross(a, b)), a @ b)
        return 0.5 * p[0] * (th - p[1]) ** 2
    return p[0] * (1.0 + np.cos(p[1] * dihedral(u) - p[2]))


def dihedral(u):
    b1, b2, b3 = u[1] - u[0], u[2] - u[1], u[3] - u[2]
    m, n = np.cross(b1, b2), np.cross(b2, b3)
    return np.arctan2(np.linalg.norm(b2) * (b1 @ n), m @ n)


def term_forces(kind, u, p):
    """(energy, forces (n_atoms, 3)) of one term at unwrapped positions u"""
    if kind == BOND:
        d = u[1] - u[0]
        r = np.linalg.norm(d)
        g = p[0] * (r - p[1]) / r if r > 0 else 0.0
        f1 = -g * d
        return 0.5 * p[0] * (r - p[1]) ** 2, np.array([-f1, f1])
    if kind == ANGLE:
        a, b = u[0] - u[1], u[2] - u[1]
        c = np.cross(a, b)
        cn = np.linalg.norm(c)
        th = np.arctan2(cn, a @ b)
        dU = p[0] * (th - p[1])
        if cn < 1e-300:                                      # straight, folded or a zero arm: no direction, no force
            return 0.5 * p[0] * (th - p[1]) ** 2, np.zeros((3, 3))
        fi = -dU * np.cross(a, c) / ((a @ a) * cn)
        fk = dU * np.cross(b, c) / ((b @ b) * cn)
        return 0.5 * p[0] * (th - p[1]) ** 2, np.array([fi, -fi - fk, fk])
    b1, b2, b3 = u[1] - u[0], u[2] - u[1], u[3] - u[2]
    m, n = np.cross(b1, b2), np.cross(b2, b3)
    b2n = np.linalg.norm(b2)
    phi = np.arctan2(b2n * (b1 @ n), m @ n)
    dU = -p[0] * p[1] * np.sin(p[1] * phi - p[2])
    if min(m @ m, n @ n, b2 @ b2) < 1e-300:              # a collinear bond pair or b2 = 0: phi is undefined, no force
        return p[0] * (1.0 + np.cos(p[1] * phi - p[2])), np.zeros((4, 3))
    gi = -b2n / (m @ m) * m                              # d phi / d x_i
    gl = b2n / (n @ n) * n                               # d phi / d x_l
    s1, s3 = (b1 @ b2) / (b2 @ b2), (b3 @ b2) / (b2 @ b2)
    gj = -(1.0 + s1) * gi + s3 * gl
    gk = -gi - gl - gj
    return p[0] * (1.0 + np.cos(p[1] * phi - p[2])), -dU * np.array([gi, gj, gk, gl])


def bonded(x, L, terms):
    """terms: list of (kind, atoms (n, k) int, params (n, m)).  Returns per-atom forces (N, 3), energies (N,), virials (N,)
    and tensors (N, 6)."""
    x = np.asarray(x, dtype=np.float64)
    N = x.shape[0]
    f, e, w, t = np.zeros((N, 3)), np.zeros(N), np.zeros(N), np.zeros((N, 6))
    for kind, atoms, params in terms:
        atoms = np.asarray(atoms).reshape(-1, ATOMS[kind])
        params = np.asarray(params, dtype=np.float64).reshape(len(atoms), -1)
        for idx, p in zip(atoms, params):
            u = unwrapped(x, idx, L)
            U, F = term_forces(kind, u, p)
            T = u.T @ F
            T = 0.5 * (T + T.T)
            share = 1.0 / len(idx)
            for a, g in enumerate(idx):
                f[g] += F[a]
                e[g] += share * U
                w[g] += share * np.trace(T)
                t[g] += share * np.array([T[0, 0], T[1, 1], T[2, 2], T[0, 1], T[0, 2], T[1, 2]])
    return f, e, w, t


def total_energy(x, L, terms):
    E = 0.0
    for kind, atoms, params in terms:
        atoms = np.asarray(atoms).reshape(-1, ATOMS[kind])
        for idx, p in zip(atoms, np.asarray(params, dtype=np.float64).reshape(len(atoms), -1)):
            E += term_energy(kind, unwrapped(x, idx, L), p)
    return E
