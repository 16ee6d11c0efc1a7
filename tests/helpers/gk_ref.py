"""Host yardstick of the Green-Kubo observables (include/emdee_hip.h: emdee_md_set_gk).  Plain numpy fp64; it never calls the
library.

The nine words of a sample: words 0-5 from the twelve sums of the pressure entry (W then K, each xx, yy, zz, xy, xz, yz), S = K + W:
S_xy, S_xz, S_yz, (S_xx - S_yy) / 2, (S_yy - S_zz) / 2, trace(S) / 3; words 6-8 the heat flux

    J = sum_i (k_i + e_i) v_i + 1/2 sum_{i != j} r_ij (f_ij . v_i),     k_i = m_i v_i^2 / 2, e_i = 1/2 sum_j u_ij,

r_ij = r_i - r_j the minimum image and f_ij the force on i from j.  heat_flux_pairs forms it from the pairs directly;
heat_flux_fields takes the per-atom energies and tensors (tests/helpers/ortho_ref.py: nonbonded) as the engine does,
J = sum (k + e) v + sum W . v -- tests/test_gk_ref_host.py holds the two against each other and J against the centred difference of
sum (k + e) x on an open box.

correlate is the brute-force sum over all pairs of samples at most n_lags - 1 apart."""
import numpy as np

from . import coulomb_ref as cr
from . import ortho_ref as oref
from . import virial_tensor_ref as vt

WORDS, STRESS_WORDS = 9, 6


def stress_words(sums12):
    """words 0-5 from the twelve sums, in the order of operations of include/emdee_hip.h"""
    t = np.asarray(sums12, dtype=np.float64)
    sxx, syy, szz = t[6] + t[0], t[7] + t[1], t[8] + t[2]
    return np.array([t[9] + t[3], t[10] + t[4], t[11] + t[5], 0.5 * (sxx - syy), 0.5 * (syy - szz), (sxx + syy + szz) / 3.0])


def masses(inv_mass, N):
    if inv_mass is None:
        return np.ones(N)
    im = np.asarray(inv_mass, dtype=np.float64)
    return np.where(im != 0.0, 1.0 / np.where(im != 0.0, im, 1.0), 0.0)


def heat_addends(vel, e, t, inv_mass=None):
    """(N, 3, 4): per atom and axis a the four addends (k + e) v_a, W_ax v_x, W_ay v_y, W_az v_z"""
    v = np.asarray(vel, dtype=np.float64)
    N = v.shape[0]
    k = 0.5 * masses(inv_mass, N) * (v * v).sum(axis=1)
    full = np.empty((N, 3, 3))
    for c, (a, b) in enumerate(vt.COMPONENTS):
        full[:, a, b] = full[:, b, a] = np.asarray(t, dtype=np.float64)[:, c]
    out = np.empty((N, 3, 4))
    out[:, :, 0] = (k + np.asarray(e, dtype=np.float64))[:, None] * v
    out[:, :, 1:] = full * v[:, None, :]
    return out


def heat_flux_fields(vel, e, t, inv_mass=None):
    """(J (3,), A (3,)): the heat flux from per-atom energies and tensors, and the sum of its absolute addends"""
    a = heat_addends(vel, e, t, inv_mass)
    return a.sum(axis=(0, 2)), np.abs(a).sum(axis=(0, 2))


def heat_flux_pairs(pos, vel, lengths, periodic, rc, rs, atoms, inv_mass=None, charges=None, coulomb_k=1.0, eps_rf=np.inf):
    """J (3,) from the pairs directly: sum (k_i + e_i) v_i + 1/2 sum_{i != j} r_ij (f_ij . v_i)"""
    pos, v = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    N = pos.shape[0]
    i, j, d = vt.pairs_in_range(pos, lengths, periodic, rc, margin=0.0)
    r2 = np.einsum("ij,ij->i", d, d)
    hs, te = oref.lj_fields(atoms)
    E, W = vt.pair_energy_virial(r2, rc, rs, hs[i], te[i], hs[j], te[j])
    if charges is not None:
        q = np.asarray(charges, dtype=np.float64)
        U, Wc = cr.pair_energy_virial(np.sqrt(r2), coulomb_k * q[i] * q[j], rc, eps_rf)
        E, W = E + U, W + Wc
    f = (W / r2)[:, None] * d                                # the force on i from j; on j from i it is -f, and r_ji = -d
    e = np.bincount(i, 0.5 * E, minlength=N) + np.bincount(j, 0.5 * E, minlength=N)
    k = 0.5 * masses(inv_mass, N) * (v * v).sum(axis=1)
    convective = ((k + e)[:, None] * v).sum(axis=0)
    # each unordered pair stands for (i, j) and (j, i): d (f . v_i) + (-d) (-f . v_j)
    virial = 0.5 * (d * (np.einsum("ij,ij->i", f, v[i]) + np.einsum("ij,ij->i", f, v[j]))[:, None]).sum(axis=0)
    return convective + virial


def energy_moment(pos, vel, lengths, periodic, rc, rs, atoms, inv_mass=None):
    """sum_i (k_i + e_i) x_i (3,): on an open box its time derivative is J"""
    pos, v = np.asarray(pos, dtype=np.float64), np.asarray(vel, dtype=np.float64)
    lo = pos.min(axis=0) - 1.0
    out = oref.nonbonded(pos, lo, np.asarray(lengths, dtype=np.float64), periodic, rc, rs, atoms)
    k = 0.5 * masses(inv_mass, pos.shape[0]) * (v * v).sum(axis=1)
    return ((k + out["e"])[:, None] * pos).sum(axis=0)


def correlate(samples, n_lags):
    """dict(sums (n_lags, 9), totals (9), counts (n_lags), abs_sums, abs_totals, terms (n_lags)) of the brute-force enumeration over
    the recorded samples A(0) ... A(n - 1): sums[l][w] = sum_{s >= l} A_w(s) A_w(s - l); abs_*: the same sums of absolute addends"""
    A = np.asarray(samples, dtype=np.float64).reshape(-1, WORDS)
    n = A.shape[0]
    sums, abs_sums, counts = np.zeros((n_lags, WORDS)), np.zeros((n_lags, WORDS)), np.zeros(n_lags, dtype=np.int64)
    for s in range(n):
        for so in range(s + 1):
            l = s - so
            if l >= n_lags:
                continue
            sums[l] += A[s] * A[so]
            abs_sums[l] += np.abs(A[s] * A[so])
            counts[l] += 1
    return dict(sums=sums, totals=A.sum(axis=0) if n else np.zeros(WORDS), counts=counts, abs_sums=abs_sums,
                abs_totals=np.abs(A).sum(axis=0) if n else np.zeros(WORDS))


def bound(ref):
    """(sums bound (n_lags, 9), totals bound (9)): 2 n 2^-53 sum |addends| with n the number of addends -- a sum of n addends in any
    order is within (n - 1) 2^-53 (1 + ...) of the exact one, the product of an addend adds one rounding more (none where the device
    contracts it into the sum), and numpy's own sum carries as much again"""
    n = np.maximum(ref["counts"], 1)[:, None].astype(np.float64)
    total_n = float(max(int(ref["counts"][0]), 1))
    return 2.0 * n * 2.0 ** -53 * ref["abs_sums"], 2.0 * total_n * 2.0 ** -53 * ref["abs_totals"]
