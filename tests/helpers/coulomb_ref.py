"""numpy fp64 restatement of the reaction-field Coulomb terms (include/emdee_hip.h emdee_md_set_coulomb), the yardstick of the
charged engines:
  k_rf = (eps_rf - 1) / ((2 eps_rf + 1) rc^3)   (1 / (2 rc^3) at eps_rf = inf),   c_rf = 1/rc + k_rf rc^2
  U = K q_i q_j (1/r + k_rf r^2 - c_rf),  W = -r dU/dr = K q_i q_j (1/r - 2 k_rf r^2),  F_i = (W / r^2) d,  d = r_i - r_j
for every pair with r^2 < rc^2 (minimum image in a periodic orthorhombic box); half of U, W and the tensor (W / r^2) d (x) d to
either atom.  Excluded pairs contribute nothing, 1-4 pairs s14 times their terms.

L is the box: one number for a cube, or the three per-axis lengths (Lx, Ly, Lz) -- every function here passes it through
box_lengths, so that the minimum image of axis a uses L[a] and nothing else."""
import numpy as np


def box_lengths(L):
    """L as the (3,) vector of per-axis lengths (a scalar is a cube)"""
    L = np.asarray(L, dtype=np.float64)
    assert L.shape in ((), (3,)), "L is one side or three per-axis lengths"
    return np.broadcast_to(L, (3,))


def rf_constants(rc, eps_rf):
    """(k_rf, c_rf)"""
    k = 0.5 / rc ** 3 if np.isinf(eps_rf) else (eps_rf - 1.0) / ((2.0 * eps_rf + 1.0) * rc ** 3)
    return k, 1.0 / rc + k * rc * rc


def pair_energy_virial(r, qq, rc, eps_rf):
    """(U, W) of pairs at distance r with K q_i q_j = qq (no cutoff test)"""
    k, c = rf_constants(rc, eps_rf)
    r = np.asarray(r, dtype=np.float64)
    return qq * (1.0 / r + k * r * r - c), qq * (1.0 / r - 2.0 * k * r * r)


def pairs_within(pos, L, rc, chunk=512):
    """every pair i < j with minimum-image distance below rc, as an (m, 2) int64 array"""
    n = pos.shape[0]
    L = box_lengths(L)
    out = []
    for a in range(0, n, chunk):
        d = pos[a:a + chunk, None, :] - pos[None, :, :]
        d -= L * np.rint(d / L)
        r2 = (d * d).sum(axis=2)
        i, j = np.nonzero(r2 < rc * rc)
        i = i + a
        keep = i < j
        out.append(np.stack([i[keep], j[keep]], axis=1))
    return np.concatenate(out).astype(np.int64) if out else np.zeros((0, 2), dtype=np.int64)


def pair_terms(pos, L, q, K, rc, eps_rf, pairs):
    """forces (n, 3), energies (n,), virials (n,), tensors (n, 6: xx, yy, zz, xy, xz, yz) of the listed pairs inside rc"""
    n = pos.shape[0]
    f, e, w, t = np.zeros((n, 3)), np.zeros(n), np.zeros(n), np.zeros((n, 6))
    pairs = np.asarray(pairs, dtype=np.int64).reshape(-1, 2)
    if pairs.shape[0] == 0:
        return f, e, w, t
    i, j = pairs[:, 0], pairs[:, 1]
    L = box_lengths(L)
    d = pos[i] - pos[j]
    d -= L * np.rint(d / L)
    r2 = (d * d).sum(axis=1)
    inside = r2 < rc * rc
    i, j, d, r2 = i[inside], j[inside], d[inside], r2[inside]
    U, W = pair_energy_virial(np.sqrt(r2), K * q[i] * q[j], rc, eps_rf)
    fv = (W / r2)[:, None] * d
    tv = (0.5 * W / r2)[:, None] * np.stack([d[:, 0] * d[:, 0], d[:, 1] * d[:, 1], d[:, 2] * d[:, 2], d[:, 0] * d[:, 1],
                                             d[:, 0] * d[:, 2], d[:, 1] * d[:, 2]], axis=1)
    for a, s in ((i, 1.0), (j, -1.0)):
        np.add.at(f, a, s * fv)
        np.add.at(e, a, 0.5 * U)
        np.add.at(w, a, 0.5 * W)
        np.add.at(t, a, tv)
    return f, e, w, t


def coulomb(pos, L, q, K, rc, eps_rf, excl=None, p14=None, s14=1.0):
    """(f, e, w, t) of every pair inside rc but the excluded ones, the 1-4 pairs scaled by s14 (excl holds neither the 1-4 pairs
    nor needs to: pass them as p14)"""
    pos = np.asarray(pos, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    out = pair_terms(pos, L, q, K, rc, eps_rf, pairs_within(pos, L, rc))
    for tab, scale in ((excl, 1.0), (p14, 1.0 - s14)):
        if tab is None or len(tab) == 0:
            continue
        sub = pair_terms(pos, L, q, K, rc, eps_rf, tab)
        out = tuple(a - scale * b for a, b in zip(out, sub))
    return out


def energy(pos, L, q, K, rc, eps_rf, excl=None, p14=None, s14=1.0):
    return coulomb(pos, L, q, K, rc, eps_rf, excl, p14, s14)[1].sum()
