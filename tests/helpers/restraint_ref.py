"""numpy restatement of the position restraints (include/emdee_hip.h: emdee_md_set_restraints), the yardstick of
tests/test_restraint_host.py and tests/test_gpu_restraints.py.  Written from the formulas of the header, not from the kernels: a
plain loop-free evaluation over all entries at once, fp64 throughout."""
import numpy as np


def terms(d, k, r0=None):
    """d, k: (n, 3); r0: (n,) or None (all zero).  Returns (U (n,), f (n, 3), T (n, 6)): the energy, the force and the symmetrised
    d (x) f in the order (xx, yy, zz, xy, xz, yz).
      r0 = 0: U = 1/2 sum_a k_a d_a^2, f_a = -k_a d_a
      r0 > 0: rho = |d| over the axes with k_a > 0, k the one non-zero constant: U = 1/2 k max(0, rho - r0)^2, f = -k (rho - r0) d_masked
              / rho outside the well, exactly 0 inside"""
    d, k = np.asarray(d, dtype=np.float64).reshape(-1, 3), np.asarray(k, dtype=np.float64).reshape(-1, 3)
    n = d.shape[0]
    r0 = np.zeros(n) if r0 is None else np.asarray(r0, dtype=np.float64).reshape(n)
    U = 0.5 * (k * d * d).sum(axis=1)
    f = -k * d
    flat = r0 > 0.0
    if flat.any():
        on = k[flat] > 0.0
        dm = np.where(on, d[flat], 0.0)
        rho = np.sqrt((dm * dm).sum(axis=1))
        kk = k[flat].max(axis=1)
        out = rho > r0[flat]
        s = np.where(out, rho - r0[flat], 0.0)
        U[flat] = 0.5 * kk * s * s
        with np.errstate(divide="ignore", invalid="ignore"):
            c = np.where(out, -kk * s / np.where(out, rho, 1.0), 0.0)
        f[flat] = c[:, None] * dm
    T = np.stack([d[:, 0] * f[:, 0], d[:, 1] * f[:, 1], d[:, 2] * f[:, 2], 0.5 * (d[:, 0] * f[:, 1] + d[:, 1] * f[:, 0]),
                  0.5 * (d[:, 0] * f[:, 2] + d[:, 2] * f[:, 0]), 0.5 * (d[:, 1] * f[:, 2] + d[:, 2] * f[:, 1])], axis=1)
    return U, f, T


def planes(n_atoms, atoms, x, ref, k, r0=None):
    """The restraint part of an engine's per-atom outputs: x (n_atoms, 3) unwrapped positions, atoms (n,) ids, ref, k (n, 3).
    Returns (forces (n_atoms, 3), energies (n_atoms,), virials (n_atoms,), tensors (n_atoms, 6)): an atom owns its whole term."""
    atoms = np.asarray(atoms, dtype=np.int64).reshape(-1)
    U, f, T = terms(np.asarray(x, dtype=np.float64)[atoms] - np.asarray(ref, dtype=np.float64), k, r0)
    F, E, W, V = np.zeros((n_atoms, 3)), np.zeros(n_atoms), np.zeros(n_atoms), np.zeros((n_atoms, 6))
    F[atoms], E[atoms], W[atoms], V[atoms] = f, U, T[:, :3].sum(axis=1), T
    return F, E, W, V


def sums(atoms, x, ref, k, r0=None):
    """emdee_md_restraint_sums: [sum U, sum T (6), max |d|]"""
    atoms = np.asarray(atoms, dtype=np.int64).reshape(-1)
    d = np.asarray(x, dtype=np.float64)[atoms] - np.asarray(ref, dtype=np.float64)
    U, _, T = terms(d, k, r0)
    return np.concatenate([[U.sum()], T.sum(axis=0), [np.sqrt((d * d).sum(axis=1)).max() if len(atoms) else 0.0]])


def scale_ref(ref, lo, mu):
    """the references after a box scale: lo + mu (ref - lo) per axis"""
    return np.asarray(lo, dtype=np.float64) + np.asarray(mu, dtype=np.float64) * (np.asarray(ref, dtype=np.float64) - np.asarray(lo, dtype=np.float64))
